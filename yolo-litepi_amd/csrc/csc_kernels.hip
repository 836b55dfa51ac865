// Colour conversion at the pipeline's front door: NV12 video frames (a full-resolution Y plane followed by a
// half-resolution interleaved UV plane) -> the packed uint8 BGR frames every downstream kernel reads.  Limited-range YCbCr in
// 20-bit fixed point, the arithmetic OpenCV publishes for COLOR_YUV2BGR_NV12 (include/litepi.h, lp_frame_format).
#include "common.h"
#include "kernels.h"
#include <type_traits>

namespace lp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));   // same 16 bytes at any address: the compiler picks a legal access

// CY, CVR, CUG, CVG, CUB per lp_csc
static const CscCoef kCscCoef[2] = {
    {1220542, 1673527, 409993, 852492, 2116026},   // LP_CSC_BT601_LIMITED (cv2's constants)
    {1220542, 1880097, 223347, 558891, 2214593},   // LP_CSC_BT709_LIMITED
};

// Every product has a coefficient below 2^22 and a sample difference within +-255: both fit 24 bits, so the full-rate 24-bit
// multiply gives the exact int32 product (the 32-bit integer multiply issues at a quarter of that rate).
// clamp(v >> 20, 0, 255), written as clamp-then-shift (the same value: the bounds are multiples of 2^20 less one).  The
// shift-then-clamp form is matched to gfx950's packed shift-and-saturate instruction, whose result came back from the
// hardware with foreign upper 16 bits under the toolchain this was developed with (tests/test_gpu_pixfmt.py caught it).
__device__ __forceinline__ int clamp_u8(int v) { return min(max(v, 0), (256 << 20) - 1) >> 20; }

// one pixel: luma byte Y with the chroma terms of its 2x2 block -> B | G << 8 | R << 16
__device__ __forceinline__ uint32_t csc_pixel(int Y, int rv, int guv, int bu, int cy) {
  const int y = __mul24(max(Y - 16, 0), cy) + (1 << 19);
  return (uint32_t)clamp_u8(y + bu) | ((uint32_t)clamp_u8(y + guv) << 8) | ((uint32_t)clamp_u8(y + rv) << 16);
}

// 16 pixels of one row (luma bytes in yv, their 8 chroma terms in rv / guv / bu) -> 48 BGR bytes as three 16-byte words
__device__ __forceinline__ void csc_row16(const u32x4 yv, const int* rv, const int* guv, const int* bu, int cy, u32x4* out) {
  uint32_t w[12];
#pragma unroll
  for (int q = 0; q < 4; ++q) {   // 4 pixels = 12 bytes = 3 words
    uint32_t p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * q + k;
      p[k] = csc_pixel((int)((yv[q] >> (8 * k)) & 0xffu), rv[i >> 1], guv[i >> 1], bu[i >> 1], cy);
    }
    w[3 * q + 0] = p[0] | (p[1] << 24);
    w[3 * q + 1] = (p[1] >> 8) | (p[2] << 16);
    w[3 * q + 2] = (p[2] >> 16) | (p[3] << 8);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) out[k] = u32x4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
}

// ------------------------------------------------------------------------------------
// A thread owns a 2-row x 16-pixel block: two 16-byte Y loads, ONE 16-byte UV load shared by both rows, and 2 x 48 bytes of
// BGR.  blockIdx.y is the frame (geometry from the device table, frames of individual sizes in one launch),
// blockIdx.x * 256 + threadIdx.x the block inside the frame, row-pair major.  The 48-byte runs leave as 16-byte stores after
// an exchange through LDS that makes each store instruction contiguous across the wave (stored straight from the owning
// lanes, 48 B apart, the kernel ran at 5.1 instead of 6.2 TB/s: DESIGN.md 6c).  ALIGNED: every address of the frame's full
// blocks is a multiple of 16 (bases, pitch and 3 * W); otherwise the same 16-byte accesses go out through an align-1 type.
// The last block of a row whose width is not a multiple of 16 is done byte by byte: nothing outside the frame is read or
// written.
// ------------------------------------------------------------------------------------
// the block's arithmetic on samples in registers: 2 x 16 luma bytes, 8 (U, V) byte pairs
__device__ __forceinline__ void csc_block_regs(const u32x4 ya, const u32x4 yb, const u32x4 uv, const CscCoef k, u32x4* o0, u32x4* o1) {
  int rv[8], guv[8], bu[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t wd = uv[j >> 1] >> (16 * (j & 1));
    const int u = (int)(wd & 0xffu) - 128, v = (int)((wd >> 8) & 0xffu) - 128;
    rv[j] = __mul24(k.cvr, v); guv[j] = -__mul24(k.cvg, v) - __mul24(k.cug, u); bu[j] = __mul24(k.cub, u);
  }
  csc_row16(ya, rv, guv, bu, k.cy, o0);
  csc_row16(yb, rv, guv, bu, k.cy, o1);
}

template <bool ALIGNED>
__device__ __forceinline__ void csc_block(const uint8_t* __restrict__ y0p, const uint8_t* __restrict__ y1p, const uint8_t* __restrict__ uvp,
                                          const CscCoef k, u32x4* o0, u32x4* o1) {
  typedef typename std::conditional<ALIGNED, u32x4, u32x4_u>::type V;
  const u32x4 ya = *reinterpret_cast<const V*>(y0p), yb = *reinterpret_cast<const V*>(y1p), uv = *reinterpret_cast<const V*>(uvp);
  csc_block_regs(ya, yb, uv, k, o0, o1);
}

// The planes of a decoder surface are addresses read from a table: without the address space in the type the compiler has to
// take them for flat addresses.  They are device memory by contract (include/litepi.h lp_surface).
typedef const __attribute__((address_space(1))) uint8_t* gmem_u8;

template <bool ALIGNED>
__device__ __forceinline__ u32x4 load16_global(gmem_u8 p) {
  typedef typename std::conditional<ALIGNED, u32x4, u32x4_u>::type V;
  return *(const __attribute__((address_space(1))) V*)p;
}

// 16 samples of 16 bits (32 bytes at p) -> their 16 high bytes: one byte permute per two words, no shift per sample
template <bool ALIGNED>
__device__ __forceinline__ u32x4 load_high_bytes(gmem_u8 p) {
  const u32x4 a = load16_global<ALIGNED>(p), b = load16_global<ALIGNED>(p + 16);
  // selector bytes 0..3 address the second operand, 4..7 the first: bytes 1 and 3 of the low word, then of the high word
  return u32x4{__builtin_amdgcn_perm(a[1], a[0], 0x07050301u), __builtin_amdgcn_perm(a[3], a[2], 0x07050301u),
               __builtin_amdgcn_perm(b[1], b[0], 0x07050301u), __builtin_amdgcn_perm(b[3], b[2], 0x07050301u)};
}

__global__ __launch_bounds__(256) void nv12_to_bgr_kernel(const uint8_t* __restrict__ src, const CscFrame* __restrict__ frames,
                                                          uint8_t* __restrict__ dst, const CscCoef k) {
  // the 48-byte runs of a wave's 64 blocks are exchanged through LDS so that each store instruction writes 16-byte chunks
  // that are consecutive across the lanes (1 KB per instruction where the blocks are neighbours in a row), not 48 B apart
  __shared__ u32x4 xch[2][256 * 3];
  const CscFrame f = frames[blockIdx.y];
  const int cpr = (f.w + 15) >> 4;   // blocks per row pair
  const int nblk = cpr * (f.h >> 1);
  const int tid = threadIdx.x, idx = blockIdx.x * 256 + tid;
  const int r = idx / cpr, c = idx - r * cpr;
  const bool valid = idx < nblk, full = valid && 16 * c + 16 <= f.w;
  const uint8_t* yp = src + f.src_off + (long)(2 * r) * f.pitch + 16 * c;
  const uint8_t* uvp = src + f.src_off + f.uv_off + (long)r * f.pitch + 16 * c;
  if (full) {
    u32x4 o0[3], o1[3];
    if (f.aligned) csc_block<true>(yp, yp + f.pitch, uvp, k, o0, o1);
    else csc_block<false>(yp, yp + f.pitch, uvp, k, o0, o1);
#pragma unroll
    for (int i = 0; i < 3; ++i) { xch[0][3 * tid + i] = o0[i]; xch[1][3 * tid + i] = o1[i]; }
  } else if (valid) {   // 2 .. 14 pixels (W is even): byte by byte, straight to memory
    uint8_t* d0 = dst + f.dst_off + (long)(2 * r) * f.w * 3 + 48 * c;
    uint8_t* d1 = d0 + (long)f.w * 3;
    const int n = f.w - 16 * c;
    for (int i = 0; i < n; i += 2) {
      const int u = (int)uvp[i] - 128, v = (int)uvp[i + 1] - 128;
      const int rv = __mul24(k.cvr, v), guv = -__mul24(k.cvg, v) - __mul24(k.cug, u), bu = __mul24(k.cub, u);
#pragma unroll
      for (int row = 0; row < 2; ++row) {
        const uint8_t* ys = row ? yp + f.pitch : yp;
        uint8_t* d = row ? d1 : d0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const uint32_t p = csc_pixel(ys[i + e], rv, guv, bu, k.cy);
          d[3 * (i + e) + 0] = (uint8_t)p; d[3 * (i + e) + 1] = (uint8_t)(p >> 8); d[3 * (i + e) + 2] = (uint8_t)(p >> 16);
        }
      }
    }
  }
  __syncthreads();
  const int wbase = tid & ~63, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int m = 64 * j + lane;           // chunk of the wave's 192: part m % 3 of the block of lane m / 3
    const int owner = m / 3, part = m - 3 * owner;
    const int oidx = blockIdx.x * 256 + wbase + owner;
    const int orow = oidx / cpr, oc = oidx - orow * cpr;
    if (oidx < nblk && 16 * oc + 16 <= f.w) {
      uint8_t* d = dst + f.dst_off + (long)(2 * orow) * f.w * 3 + 48 * oc + 16 * part;
      const u32x4 a = xch[0][3 * wbase + m], b = xch[1][3 * wbase + m];
      if (f.aligned) {
        *reinterpret_cast<u32x4*>(d) = a;
        *reinterpret_cast<u32x4*>(d + (long)f.w * 3) = b;
      } else {
        *reinterpret_cast<u32x4_u*>(d) = a;
        *reinterpret_cast<u32x4_u*>(d + (long)f.w * 3) = b;
      }
    }
  }
}

void launch_nv12_to_bgr(const uint8_t* src, const CscFrame* frames, uint8_t* dst, int B, int max_blocks, int matrix, hipStream_t st) {
  if (B <= 0 || max_blocks <= 0) return;
  LP_CHECK(matrix == LP_CSC_BT601_LIMITED || matrix == LP_CSC_BT709_LIMITED, LP_ERR_ARG, "unknown colour matrix %d", matrix);
  dim3 grid(ceil_div(max_blocks, 256), B);
  LP_LAUNCH(nv12_to_bgr_kernel, grid, dim3(256), 0, st, src, frames, dst, kCscCoef[matrix]);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// Decoder surfaces: the same work split, arithmetic and LDS exchange as nv12_to_bgr_kernel, on frames whose
// two planes are absolute addresses with a pitch each, read from the one device table of the handle.  P010: 16-bit samples
// of which the high byte is taken (2 x 32 B of luma and 32 B of chroma per block), else 8-bit NV12 samples.  The frame's
// `aligned` flag picks the access type as there; the last block of a row whose width is no multiple of 16 goes byte by byte.
// Nothing outside a plane's pitch x rows is read, nothing outside the frame's H * W * 3 bytes is written.
// ------------------------------------------------------------------------------------
template <bool P010>
__global__ __launch_bounds__(256) void surfaces_to_bgr_kernel(const SurfFrame* __restrict__ frames, uint8_t* __restrict__ dst, const CscCoef k) {
  constexpr int BPS = P010 ? 2 : 1;   // bytes per sample
  __shared__ u32x4 xch[2][256 * 3];
  const SurfFrame f = frames[blockIdx.y];
  const int cpr = (f.w + 15) >> 4;   // blocks per row pair
  const int nblk = cpr * (f.h >> 1);
  if ((int)blockIdx.x * 256 >= nblk) return;   // the grid is sized for the call's largest frame (uniform: before the barrier)
  const int tid = threadIdx.x, idx = blockIdx.x * 256 + tid;
  const int r = idx / cpr, c = idx - r * cpr;
  const bool valid = idx < nblk, full = valid && 16 * c + 16 <= f.w;
  const gmem_u8 yp = (gmem_u8)f.y + (long)(2 * r) * f.pitch_y + 16 * BPS * c;
  const gmem_u8 uvp = (gmem_u8)f.uv + (long)r * f.pitch_uv + 16 * BPS * c;
  if (full) {
    u32x4 o0[3], o1[3];
    if (P010) {
      if (f.aligned) csc_block_regs(load_high_bytes<true>(yp), load_high_bytes<true>(yp + f.pitch_y), load_high_bytes<true>(uvp), k, o0, o1);
      else csc_block_regs(load_high_bytes<false>(yp), load_high_bytes<false>(yp + f.pitch_y), load_high_bytes<false>(uvp), k, o0, o1);
    } else {
      if (f.aligned) csc_block_regs(load16_global<true>(yp), load16_global<true>(yp + f.pitch_y), load16_global<true>(uvp), k, o0, o1);
      else csc_block_regs(load16_global<false>(yp), load16_global<false>(yp + f.pitch_y), load16_global<false>(uvp), k, o0, o1);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { xch[0][3 * tid + i] = o0[i]; xch[1][3 * tid + i] = o1[i]; }
  } else if (valid) {   // 2 .. 14 pixels (W is even): sample by sample, straight to memory
    uint8_t* d0 = dst + f.dst_off + (long)(2 * r) * f.w * 3 + 48 * c;
    uint8_t* d1 = d0 + (long)f.w * 3;
    const int n = f.w - 16 * c;
    constexpr int HI = BPS - 1;   // the byte of a sample that is read
    for (int i = 0; i < n; i += 2) {
      const int u = (int)uvp[BPS * i + HI] - 128, v = (int)uvp[BPS * (i + 1) + HI] - 128;
      const int rv = __mul24(k.cvr, v), guv = -__mul24(k.cvg, v) - __mul24(k.cug, u), bu = __mul24(k.cub, u);
#pragma unroll
      for (int row = 0; row < 2; ++row) {
        const gmem_u8 ys = row ? yp + f.pitch_y : yp;
        uint8_t* d = row ? d1 : d0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const uint32_t p = csc_pixel(ys[BPS * (i + e) + HI], rv, guv, bu, k.cy);
          d[3 * (i + e) + 0] = (uint8_t)p; d[3 * (i + e) + 1] = (uint8_t)(p >> 8); d[3 * (i + e) + 2] = (uint8_t)(p >> 16);
        }
      }
    }
  }
  __syncthreads();
  const int wbase = tid & ~63, lane = tid & 63;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int m = 64 * j + lane;           // chunk of the wave's 192: part m % 3 of the block of lane m / 3
    const int owner = m / 3, part = m - 3 * owner;
    const int oidx = blockIdx.x * 256 + wbase + owner;
    const int orow = oidx / cpr, oc = oidx - orow * cpr;
    if (oidx < nblk && 16 * oc + 16 <= f.w) {
      uint8_t* d = dst + f.dst_off + (long)(2 * orow) * f.w * 3 + 48 * oc + 16 * part;
      const u32x4 a = xch[0][3 * wbase + m], b = xch[1][3 * wbase + m];
      if (f.aligned) {
        *reinterpret_cast<u32x4*>(d) = a;
        *reinterpret_cast<u32x4*>(d + (long)f.w * 3) = b;
      } else {
        *reinterpret_cast<u32x4_u*>(d) = a;
        *reinterpret_cast<u32x4_u*>(d + (long)f.w * 3) = b;
      }
    }
  }
}

void launch_surfaces_to_bgr(const SurfFrame* frames, uint8_t* dst, int B, int max_blocks, bool p010, int matrix, hipStream_t st) {
  if (B <= 0 || max_blocks <= 0) return;
  LP_CHECK(matrix == LP_CSC_BT601_LIMITED || matrix == LP_CSC_BT709_LIMITED, LP_ERR_ARG, "unknown colour matrix %d", matrix);
  dim3 grid(ceil_div(max_blocks, 256), B);
  if (p010) LP_LAUNCH(surfaces_to_bgr_kernel<true>, grid, dim3(256), 0, st, frames, dst, kCscCoef[matrix]);
  else LP_LAUNCH(surfaces_to_bgr_kernel<false>, grid, dim3(256), 0, st, frames, dst, kCscCoef[matrix]);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
