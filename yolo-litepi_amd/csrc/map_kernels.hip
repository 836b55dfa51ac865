// Mapped views (include/litepi.h "mapped views"): the gather that fills a view through its remap table and the
// kernel that carries the view's candidates back to the frame.  Both are front ends of the rules in view_map.h, which the host
// entry points (lp_map_render, lp_map_box) share with them.
#include "common.h"
#include "kernels.h"
#include "view_map.h"
#include <algorithm>

namespace lp {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------
// dst[slot0 + n] = the frame seen through maps[n].  One thread per four view pixels of a row (S % 4 == 0): its 32 table bytes
// are two 16-byte loads of the coalesced stream, its 12 output bytes three dword stores.  The taps are byte gathers through
// vm_tap: a tap outside the frame is predicated to 114 and not fetched, and no load is wider than the byte it needs, so the
// frame's last pixel is read by no load that passes it.  Neighbouring view pixels of any sensible map read neighbouring
// frame bytes: the cache hierarchy carries the gathers.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_views_kernel(const uint8_t* __restrict__ src, const MapSlot* __restrict__ maps,
                                                        uint8_t* __restrict__ dst, int slot0, int S) {
  const int n = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;   // pixels 4q .. 4q + 3
  if (q >= S * S / 4) return;
  const MapSlot m = maps[n];
  const i32x4* tab = reinterpret_cast<const i32x4*>(m.fixed) + 2L * q;
  const i32x4 a = tab[0], b = tab[1];
  const uint8_t* frame = src + m.frame_off;
  union { uint8_t u8[12]; uint32_t u32[3]; } px;
  vm_pixel(frame, m.H, m.W, a[0], a[1], px.u8);
  vm_pixel(frame, m.H, m.W, a[2], a[3], px.u8 + 3);
  vm_pixel(frame, m.H, m.W, b[0], b[1], px.u8 + 6);
  vm_pixel(frame, m.H, m.W, b[2], b[3], px.u8 + 9);
  uint32_t* out = reinterpret_cast<uint32_t*>(dst + (long)(slot0 + n) * S * S * 3) + 3L * q;
  out[0] = px.u32[0]; out[1] = px.u32[1]; out[2] = px.u32[2];
}

void launch_map_views(const uint8_t* src, const MapSlot* maps, uint8_t* dst, int slot0, int n, int S, hipStream_t st) {
  if (n <= 0) return;
  LP_CHECK(S % 4 == 0 && S >= 4, LP_ERR_ARG, "mapped views need det_input %% 4 == 0");
  dim3 grid(ceil_div(S * S / 4, 256), n);
  LP_LAUNCH(map_views_kernel, grid, dim3(256), 0, st, src, maps, dst, slot0, S);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// The candidates of mapped slot slot0 + n, decoded as for a crop of an S x S image, go to frame coordinates through maps[n]
// (vm_box), in place; score, class and anchor stay.  The slot's count is read on the device: nothing waits for the host.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_candidates_kernel(const MapSlot* __restrict__ maps, Cand* __restrict__ cand,
                                                             const int* __restrict__ cand_count, int slot0, int A, int S) {
  const int n = blockIdx.y, slot = slot0 + n;
  int cnt = cand_count[slot];
  cnt = cnt > A ? A : cnt;
  const MapSlot m = maps[n];
  Cand* list = cand + (long)slot * A;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < cnt; k += gridDim.x * 256) {
    const float box[4] = {list[k].x1, list[k].y1, list[k].x2, list[k].y2};
    float out[4];
    vm_box(m.fixed, S, m.H, m.W, box, out);
    list[k].x1 = out[0]; list[k].y1 = out[1]; list[k].x2 = out[2]; list[k].y2 = out[3];
  }
}

void launch_map_candidates(const MapSlot* maps, Cand* cand, const int* cand_count, int slot0, int n, int A, int S, hipStream_t st) {
  if (n <= 0) return;
  LP_CHECK(S >= 2 && A >= 1, LP_ERR_ARG, "mapped candidates: det_input %d, %d anchors", S, A);
  dim3 grid(ceil_div(std::min(A, 1024), 256), n);
  LP_LAUNCH(map_candidates_kernel, grid, dim3(256), 0, st, maps, cand, cand_count, slot0, A, S);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
