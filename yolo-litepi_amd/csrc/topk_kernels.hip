// Top-k of the classifier's distribution per detection (include/litepi.h, lp_topk).  Two plain launches in
// stream order: the clear writes the empty record into all B * max_det records of the call's frames (an ROI-indexed kernel
// cannot reach the records no ROI names), the select behind it scatters the top-k of every classified ROI to its
// (frame, slot).  Two launches rule out a race between clearing and scattering by construction.
// Select: ONE WAVE per ROI.  Lane l owns the classes l, l + 64, l + 128, ...; the row of probabilities is read from memory
// once into LDS (each lane re-reads only what it wrote: no fence is needed), then k rounds of a wave-wide maximum over the
// 64-bit keys of topk_select.h, round j restricted to keys below round j - 1's winner.  After the butterfly every lane holds
// every winner, so lanes 0..3 write the record's four 16-byte quarters.  Integer operations only.
#include "common.h"
#include "kernels.h"
#include "topk_select.h"

namespace lp {

#define TOPK_WAVES 4                  // waves (ROIs in flight) per workgroup
#define TOPK_LDS_NC 1024              // classes of a row staged in LDS; a longer row is re-read from L2 every round

typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void topk_clear_kernel(i32x4* out, int n_quarters) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_quarters) return;
  const int v = (t & 3) < 2 ? -1 : 0;   // quarters 0, 1: cls = -1; quarters 2, 3: prob = 0
  out[t] = i32x4{v, v, v, v};
}

template <bool STAGED>
__device__ __forceinline__ void topk_one_roi(const TopkArgs& a, int r, int lane, uint32_t* s_row) {
  const int b = a.roi_img[r], slot = a.roi_slot[r];
  if (b < 0 || b >= a.B || slot < 0 || slot >= a.max_det) return;   // uniform: a record outside the call's frames is never written
  const uint32_t* row = reinterpret_cast<const uint32_t*>(a.probs) + (size_t)r * a.nc;
  if (STAGED)
    for (int c = lane; c < a.nc; c += 64) s_row[c] = row[c];
  int cls[LP_TOPK_K_MAX];
  uint32_t pb[LP_TOPK_K_MAX];
  uint64_t below = ~0ull;
#pragma unroll
  for (int j = 0; j < LP_TOPK_K_MAX; ++j) {
    uint64_t best = 0;
    if (j < a.k && below != 0) {
      for (int c = lane; c < a.nc; c += 64) best = topk_better(best, topk_key(STAGED ? s_row[c] : row[c], c), below);
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const uint64_t other = __shfl_xor(best, o);
        best = other > best ? other : best;
      }
    }
    cls[j] = best ? topk_key_class(best) : -1;
    pb[j] = best ? topk_key_bits(best) : 0u;
    below = best;
  }
  if (lane < 4) {
    i32x4 q;
    if (lane == 0) q = i32x4{cls[0], cls[1], cls[2], cls[3]};
    else if (lane == 1) q = i32x4{cls[4], cls[5], cls[6], cls[7]};
    else if (lane == 2) q = i32x4{(int)pb[0], (int)pb[1], (int)pb[2], (int)pb[3]};
    else q = i32x4{(int)pb[4], (int)pb[5], (int)pb[6], (int)pb[7]};
    reinterpret_cast<i32x4*>(a.out + (size_t)b * a.max_det + slot)[lane] = q;
  }
}

__global__ __launch_bounds__(64 * TOPK_WAVES) void topk_select_kernel(const TopkArgs a) {
  __shared__ uint32_t s_rows[TOPK_WAVES][TOPK_LDS_NC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int R = min(max(*a.total, 0), a.cap);   // the classified ROIs, read where roi_resize and the classifier read them
  const bool staged = a.nc <= TOPK_LDS_NC;
  for (int r = blockIdx.x * TOPK_WAVES + wave; r < R; r += gridDim.x * TOPK_WAVES) {
    if (staged) topk_one_roi<true>(a, r, lane, s_rows[wave]);
    else topk_one_roi<false>(a, r, lane, nullptr);
  }
}

void launch_topk_clear(lp_topk* out, int n_records, hipStream_t st) {
  if (n_records <= 0) return;
  const int n_quarters = n_records * 4;
  LP_LAUNCH(topk_clear_kernel, dim3((n_quarters + 255) / 256), dim3(256), 0, st, reinterpret_cast<i32x4*>(out), n_quarters);
  LP_HIP(hipGetLastError());
}

void launch_topk_select(const TopkArgs& a, hipStream_t st) {
  LP_CHECK(a.nc >= 1 && a.k >= 1 && a.k <= LP_TOPK_K_MAX && a.B >= 1 && a.max_det >= 1, LP_ERR_ARG, "bad top-k shape (classes %d, k %d)", a.nc, a.k);
  if (a.cap <= 0) return;
  const int grid = std::min((a.cap + TOPK_WAVES - 1) / TOPK_WAVES, 2048);
  LP_LAUNCH(topk_select_kernel, dim3(grid), dim3(64 * TOPK_WAVES), 0, st, a);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
