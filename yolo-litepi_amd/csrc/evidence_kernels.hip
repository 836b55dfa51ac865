// Evidence store: the picture launch behind the deciding inventory kernel (the rule is stated in
// include/litepi.h, lp_evidence_config).  inventory_evidence_kernel (inventory_kernels.hip) moves no pixel: it leaves one
// compact list of records (kernels.h, EvJob).  This launch does the moving: `workers` x E / EV_TH workgroups, a worker walks
// the list with the workers' stride, one band of EV_TH picture rows per workgroup.  A record's gallery -> log copy (an entry
// that closed with a best from an earlier call) comes before its frame -> gallery render (an entry still open whose final
// best lies in this call) -- in the same workgroup and over the same bytes, so a slot closed and reused within one call keeps
// the old picture in the log and gets the new one in the gallery; a record with log_pos renders frame -> log.
// A picture is the window view of the frame for a detector input of E: window_views_kernel's arithmetic (tile_kernels.hip;
// lin_coeff's fixed point over the WINDOW's size, 114 in the bars), with the window and its letterbox geometry computed
// here, on the device, from evidence_window.h.  The two source rows of every output row of the band are staged in LDS with
// aligned 16-byte loads when the window's row span fits EV_ROW_CAP; a longer row (windows beyond ~670 pixels) takes the
// per-pixel form straight from global memory, as the view gather does.  Vector stores only, no local arrays that spill.
#include "common.h"
#include "evidence_window.h"
#include "kernels.h"
#include "post_dev.h"

namespace lp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define EV_TH 8            // picture rows of a band
#define EV_ROW_CAP 2048    // bytes of one staged source row (span + alignment slack); 2 * EV_TH rows = 32 KB of LDS

struct EvSource {          // one window of one frame
  const uint8_t* im;       // the frame's first byte
  long frame_bytes;
  int pitch, x, y, w, h;
};

// The resample of a band: a thread takes four adjacent columns of one row.  STAGED: the rows come from LDS, row 2j / 2j+1 of
// `band`, where window byte b sits at s_shift[row] - b0 + b.  The offset is added to the byte index, never to the row's
// address: b0 > 0 once the down-scale passes 3x, and an LDS address that goes below its base and is widened to a generic
// pointer afterwards leaves the LDS aperture.  The two forms are instantiated apart, so LDS rows are read with LDS loads.
template <bool STAGED>
__device__ __forceinline__ void resample_band(const EvSource& sw, const EvGeom& g, bool resize, uint8_t* __restrict__ pic, int E, int oy0,
                                              const uint8_t* band, const int* s_shift, int b0) {
  const int tid = threadIdx.x;
  const int groups = E >> 2;   // E % 16 == 0
  for (int u = tid; u < EV_TH * groups; u += 256) {
    const int j = u / groups, ox = 4 * (u - j * groups), oy = oy0 + j;
    const int dy = oy - g.top;
    const bool rowin = dy >= 0 && dy < g.new_h;
    int sy = 0, ay0 = 2048, ay1 = 0;
    if (rowin) { if (resize) lin_coeff(dy, g.new_h, sw.h, sy, ay0, ay1); else sy = dy; }
    const int sy1 = sy + 1 < sw.h ? sy + 1 : sw.h - 1;
    const uint8_t *r0, *r1;   // window row sy / sy1; window byte b is r0[o0 + b] / r1[o1 + b]
    int o0 = 0, o1 = 0;
    if constexpr (STAGED) {
      r0 = band + (size_t)(2 * j) * EV_ROW_CAP;
      r1 = band + (size_t)(2 * j + 1) * EV_ROW_CAP;
      if (rowin) { o0 = s_shift[2 * j] - b0; o1 = s_shift[2 * j + 1] - b0; }
    } else {
      r0 = sw.im + (long)(sw.y + sy) * sw.pitch + 3L * sw.x;
      r1 = sw.im + (long)(sw.y + sy1) * sw.pitch + 3L * sw.x;
    }
    uint32_t out[3] = {0u, 0u, 0u};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int dx = ox + q - g.left;
      uint32_t px[3] = {114u, 114u, 114u};
      if (rowin && dx >= 0 && dx < g.new_w) {
        if (resize) {
          int sx, ax0, ax1;
          lin_coeff(dx, g.new_w, sw.w, sx, ax0, ax1);
          const int sx1 = sx + 1 < sw.w ? sx + 1 : sw.w - 1;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int h0 = r0[o0 + sx * 3 + c] * ax0 + r0[o0 + sx1 * 3 + c] * ax1;
            const int h1 = r1[o1 + sx * 3 + c] * ax0 + r1[o1 + sx1 * 3 + c] * ax1;
            const int v = (((ay0 * (h0 >> 4)) >> 16) + ((ay1 * (h1 >> 4)) >> 16) + 2) >> 2;
            px[c] = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
          }
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) px[c] = r0[o0 + dx * 3 + c];
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = 3 * q + c;
        out[b >> 2] |= px[c] << (8 * (b & 3));
      }
    }
    uint32_t* o = reinterpret_cast<uint32_t*>(pic + ((long)oy * E + ox) * 3);   // 12-byte groups: 4-byte aligned
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
  }
}

// rows oy0 .. oy0 + EV_TH - 1 of the E x E picture of `sw` into pic (the picture's first byte); the whole workgroup calls it
__device__ __forceinline__ void render_band(const EvSource& sw, uint8_t* __restrict__ pic, int E, int oy0, uint8_t* band, int* s_shift) {
  const int tid = threadIdx.x;
  const EvGeom g = evidence_geom(sw.h, sw.w, E);
  const bool resize = !(g.new_w == sw.w && g.new_h == sw.h);
  // the byte span [b0, b1) of a WINDOW row that the picture's columns read
  int b0 = 0, b1 = 0;
  {
    int sa = 0, sb = g.new_w - 1, t0, t1;
    if (resize) { lin_coeff(0, g.new_w, sw.w, sa, t0, t1); lin_coeff(g.new_w - 1, g.new_w, sw.w, sb, t0, t1); }
    const int sb1 = sb + 1 < sw.w ? sb + 1 : sw.w - 1;
    b0 = 3 * sa; b1 = 3 * (sb1 + 1);
  }
  const bool staged = b1 - b0 + 32 <= EV_ROW_CAP;   // uniform over the workgroup
  if (staged) {
    for (int r = tid >> 4; r < 2 * EV_TH; r += 16) {   // 16 threads per row; LDS row 2j / 2j+1 = window rows sy / sy1 of output row oy0 + j
      const int dy = oy0 + (r >> 1) - g.top;
      if (dy < 0 || dy >= g.new_h) continue;
      int sy, ay0, ay1;
      if (resize) lin_coeff(dy, g.new_h, sw.h, sy, ay0, ay1); else sy = dy;
      const int syr = (r & 1) ? (sy + 1 < sw.h ? sy + 1 : sw.h - 1) : sy;
      const long goff = (long)(sw.y + syr) * sw.pitch + 3L * sw.x + b0;   // byte offset of the span inside the frame
      const int shift = (int)(reinterpret_cast<uintptr_t>(sw.im + goff) & 15);
      const long gal = goff - shift;                                       // 16-byte aligned start, relative to the frame
      if ((tid & 15) == 0) s_shift[r] = shift;
      const int nchunk = min((shift + (b1 - b0) + 15) >> 4, EV_ROW_CAP >> 4);   // (`staged` sized the span: never cuts)
      for (int c = tid & 15; c < nchunk; c += 16) {
        const long o = gal + 16L * c;
        u32x4 v;
        if (o >= 0 && o + 16 <= sw.frame_bytes) {
          v = *reinterpret_cast<const u32x4*>(sw.im + o);
        } else {   // the chunk passes the frame's first or last byte: byte by byte, nothing outside the frame is touched
          v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (o + k >= 0 && o + k < sw.frame_bytes) v[k >> 2] |= (uint32_t)sw.im[o + k] << (8 * (k & 3));
        }
        *reinterpret_cast<u32x4*>(band + (size_t)r * EV_ROW_CAP + 16 * c) = v;
      }
    }
  }
  __syncthreads();
  if (staged) resample_band<true>(sw, g, resize, pic, E, oy0, band, s_shift, b0);
  else resample_band<false>(sw, g, resize, pic, E, oy0, band, s_shift, b0);
  __syncthreads();   // the band is free for the next picture of this workgroup
}

__device__ __forceinline__ EvSource source_of(const EvArgs& e, int b, int x, int y, int w, int h) {
  const ImgGeom* g = e.fgeom + b;
  EvSource s;
  s.im = e.frames + g->src_off; s.pitch = 3 * g->w; s.frame_bytes = (long)g->h * s.pitch;
  s.x = x; s.y = y; s.w = w; s.h = h;
  return s;
}

// a window the frame does not hold is never rendered (the deciding kernel makes none: this guards a frame table that
// changed between the two launches' reads, which the entry points' contract excludes)
__device__ __forceinline__ bool holds(const EvSource& s) {
  return s.w >= LP_EVIDENCE_SIDE_MIN && s.h >= LP_EVIDENCE_SIDE_MIN && s.x >= 0 && s.y >= 0 && 3L * (s.x + s.w) <= s.pitch &&
         (long)(s.y + s.h) * s.pitch <= s.frame_bytes;
}

__global__ __launch_bounds__(256) void evidence_pictures_kernel(const EvArgs e) {
  __shared__ __attribute__((aligned(16))) uint8_t band[2 * EV_TH * EV_ROW_CAP];
  __shared__ int s_shift[2 * EV_TH];
  const int oy0 = blockIdx.y * EV_TH, E = e.E;
  const size_t pic_bytes = (size_t)3 * E * E;
  const int n = min(max(*e.n_jobs, 0), e.cap_jobs);
  for (int i = blockIdx.x; i < n; i += gridDim.x) {   // uniform over the workgroup
    const u32x4* jp = reinterpret_cast<const u32x4*>(e.jobs + i);
    const u32x4 j0 = jp[0], j1 = jp[1];
    const int copy_pos = (int)j0.x, b = (int)j0.y, gal_i = (int)j1.z, log_pos = (int)j1.w;
    uint8_t* gal = gal_i >= 0 ? e.gallery + (size_t)gal_i * pic_bytes : nullptr;
    if (copy_pos >= 0 && gal) {   // gallery -> log: the band's bytes, 16 per lane
      const size_t off = (size_t)oy0 * E * 3;
      const u32x4* s = reinterpret_cast<const u32x4*>(gal + off);
      u32x4* d = reinterpret_cast<u32x4*>(e.log_pics + (size_t)copy_pos * pic_bytes + off);
      for (int q = threadIdx.x; q < EV_TH * E * 3 / 16; q += 256) d[q] = s[q];
    }
    uint8_t* dst = log_pos >= 0 ? e.log_pics + (size_t)log_pos * pic_bytes : gal;
    if (b >= 0 && dst) {
      __syncthreads();   // the band's gallery bytes are read before they are written
      const EvSource sw = source_of(e, b, (int)j0.z, (int)j0.w, (int)j1.x, (int)j1.y);
      if (holds(sw)) render_band(sw, dst, E, oy0, band, s_shift);
    }
  }
}

void launch_evidence_pictures(const EvArgs& e, int workers, hipStream_t st) {
  if (workers <= 0) return;
  LP_CHECK(e.E >= 32 && e.E <= 256 && e.E % 16 == 0, LP_ERR_ARG, "evidence pictures of side %d", e.E);
  LP_LAUNCH(evidence_pictures_kernel, dim3(workers, e.E / EV_TH), dim3(256), 0, st, e);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
