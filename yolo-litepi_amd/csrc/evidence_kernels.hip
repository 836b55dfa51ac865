// Evidence store: the picture launch behind the deciding inventory kernel (the rule is stated in
// include/litepi.h, lp_evidence_config).  inventory_evidence_kernel (inventory_kernels.hip) moves no pixel: it leaves one
// compact list of records (kernels.h, EvJob).  This launch does the moving: `workers` x E / LB_TH workgroups, a worker walks
// the list with the workers' stride, one band of LB_TH picture rows per workgroup.  A record's gallery -> log copy (an entry
// that closed with a best from an earlier call) comes before its frame -> gallery render (an entry still open whose final
// best lies in this call) -- in the same workgroup and over the same bytes, so a slot closed and reused within one call keeps
// the old picture in the log and gets the new one in the gallery; a record with log_pos renders frame -> log.
// A picture is the window view of the frame for a detector input of E: a front end of the letterbox core (letterbox_core.h)
// with the window and its placement computed here, on the device, from evidence_window.h.  The band's rows are staged in the
// 32 KB of static LDS when the window's exact row span fits EV_ROW_CAP; a longer row (windows beyond ~670 pixels) takes the
// per-pixel form straight from global memory, as the view gather does.
#include "common.h"
#include "evidence_window.h"
#include "kernels.h"

namespace lp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// The resample of a band: a thread takes four adjacent columns of one row, over the E / 4 column groups.  The staged and the
// global form are instantiated apart, so LDS rows are read with LDS loads.
template <bool STAGED>
__device__ __forceinline__ void resample_band(const LbSource& sw, const LbPlace& g, bool resize, LbSpan sp, uint8_t* __restrict__ pic, int E,
                                              int oy0, const uint8_t* band, const int* s_shift) {
  const int groups = E >> 2;   // E % 16 == 0
  for (int u = threadIdx.x; u < LB_TH * groups; u += 256) {
    const int j = u / groups, ox = 4 * (u - j * groups);
    const LbRowCoef rc = lb_row_coef(sw, g, resize, oy0 + j);
    if constexpr (STAGED)
      lb_store4(sw, g, resize, rc, pic, E, oy0 + j, ox, lb_staged_row(band, EV_ROW_CAP, s_shift, 2 * j, rc.in, sp.b0),
                lb_staged_row(band, EV_ROW_CAP, s_shift, 2 * j + 1, rc.in, sp.b0));
    else
      lb_store4(sw, g, resize, rc, pic, E, oy0 + j, ox, lb_global_row(sw, rc.sy), lb_global_row(sw, rc.sy1));
  }
}

// rows oy0 .. oy0 + LB_TH - 1 of the E x E picture of `sw` into pic (the picture's first byte); the whole workgroup calls it
__device__ __forceinline__ void render_band(const LbSource& sw, uint8_t* __restrict__ pic, int E, int oy0, uint8_t* band, int* s_shift) {
  const LbPlace g = evidence_geom(sw.h, sw.w, E);
  const bool resize = lb_resizes(sw, g);
  const LbSpan sp = lb_span(sw, g, resize, 0, g.new_w);    // the byte span of a WINDOW row that the picture's columns read
  const bool staged = sp.b1 - sp.b0 + 32 <= EV_ROW_CAP;    // uniform over the workgroup
  if (staged) lb_stage_band(sw, g, resize, sp, oy0, band, EV_ROW_CAP, s_shift);
  __syncthreads();
  if (staged) resample_band<true>(sw, g, resize, sp, pic, E, oy0, band, s_shift);
  else resample_band<false>(sw, g, resize, sp, pic, E, oy0, band, s_shift);
  __syncthreads();   // the band is free for the next picture of this workgroup
}

__device__ __forceinline__ LbSource source_of(const EvArgs& e, int b, int x, int y, int w, int h) {
  LbSource s = lb_source(e.frames, e.fgeom[b]);   // the frame, rows 3 * w bytes apart
  s.x = x; s.y = y; s.w = w; s.h = h;
  return s;
}

// a window the frame does not hold is never rendered (the deciding kernel makes none: this guards a frame table that
// changed between the two launches' reads, which the entry points' contract excludes)
__device__ __forceinline__ bool holds(const LbSource& s) {
  return s.w >= LP_EVIDENCE_SIDE_MIN && s.h >= LP_EVIDENCE_SIDE_MIN && s.x >= 0 && s.y >= 0 && 3L * (s.x + s.w) <= s.pitch &&
         (long)(s.y + s.h) * s.pitch <= s.frame_bytes;
}

__global__ __launch_bounds__(256) void evidence_pictures_kernel(const EvArgs e) {
  __shared__ __attribute__((aligned(16))) uint8_t band[2 * LB_TH * EV_ROW_CAP];
  __shared__ int s_shift[2 * LB_TH];
  const int oy0 = blockIdx.y * LB_TH, E = e.E;
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
      for (int q = threadIdx.x; q < LB_TH * E * 3 / 16; q += 256) d[q] = s[q];
    }
    uint8_t* dst = log_pos >= 0 ? e.log_pics + (size_t)log_pos * pic_bytes : gal;
    if (b >= 0 && dst) {
      __syncthreads();   // the band's gallery bytes are read before they are written
      const LbSource sw = source_of(e, b, (int)j0.z, (int)j0.w, (int)j1.x, (int)j1.y);
      if (holds(sw)) render_band(sw, dst, E, oy0, band, s_shift);
    }
  }
}

void launch_evidence_pictures(const EvArgs& e, int workers, hipStream_t st) {
  if (workers <= 0) return;
  LP_CHECK(e.E >= 32 && e.E <= 256 && e.E % 16 == 0, LP_ERR_ARG, "evidence pictures of side %d", e.E);
  LP_LAUNCH(evidence_pictures_kernel, dim3(workers, e.E / LB_TH), dim3(256), 0, st, e);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
