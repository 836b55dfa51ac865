// Sharpness and exposure of every classified detection's crop (include/litepi.h, lp_quality).  Two plain launches
// in stream order, as top-k's: the clear writes the empty record into all B * max_det records of the call's frames (an
// ROI-indexed kernel cannot reach the records no ROI names), the measure behind it writes the record of every ROI that has a crop.
// Measure: ONE WORKGROUP of 256 threads per ROI.
//   load   a thread takes 16 pixels = 48 contiguous bytes as three 16-byte loads (S % 4 == 0 makes a crop a whole number of
//          such units; at S = 64 exactly one per thread), turns them into 16 luma bytes, adds them to its exposure sums and
//          stores them as one 16-byte LDS write.  The luma plane is LINEAR in LDS (byte p = y * S + x, no row pitch), so a unit
//          that straddles two rows (3S % 16 != 0, S = 36) needs no special case.
//   tap    a thread owns one packed word (a horizontal run of 4 pixels) at a time, word j = tid, tid + 256, ...: it reads the
//          words above and below, its own and the two beside it (five ds_read_b32 at j - S/4, j + S/4, j, j - 1, j + 1) and
//          takes the 4 Laplacians from registers.  Consecutive lanes read consecutive words in every one of the five reads, so
//          a 32-lane group covers 32 distinct banks: no conflict, and no padding that would break the linear order.
//   strips the plane is held QM_LDS_BYTES at a time: rows [y0 - 1, y0 + H + 1) for the Laplacians of rows [y0, y0 + H), H a
//          multiple of 4 so that every strip STARTS on a 16-pixel unit.  Its end, 2 S further, is a unit boundary only when
//          S % 8 == 0: the loaded range is rounded up to a whole unit (qm_strip, quality_measure.h; up to 8 pixels of the row
//          behind the halo come along, and LDS has room for them).  S <= 180 is one strip; S = 224 (49 KB) is two.  What a
//          strip shares with the one before is loaded again but counted in the exposure sums once (`counted`, a unit boundary).
//   sums   integers only: per thread in registers (s2 in 64 bits), per wave by xor shuffles, across the 4 waves through LDS;
//          thread 0 turns them into the record (quality_measure.h) and writes its 32 bytes as two 16-byte stores.
#include "common.h"
#include "kernels.h"
#include "quality_measure.h"

namespace lp {

#define QM_THREADS 256
#define QM_WAVES (QM_THREADS / 64)
#define QM_LDS_BYTES LP_QM_LDS_BYTES   // luma bytes of a strip held in LDS (quality_measure.h: the strip plan)
#define QM_MAX_GRID 2048

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(lp_quality) == 32 && sizeof(QualityRec) == sizeof(lp_quality), "lp_quality is 32 bytes");

__global__ __launch_bounds__(256) void quality_clear_kernel(i32x4* out, int n_halves) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n_halves) return;
  out[t] = (t & 1) ? i32x4{0, 0, 0, 0} : i32x4{__float_as_int(-1.0f), 0, 0, 0};   // sharpness = -1, the rest zero
}

__device__ __forceinline__ long long qm_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ int qm_byte(unsigned w, int i) { return (int)((w >> (8 * i)) & 255u); }

__global__ __launch_bounds__(QM_THREADS) void quality_measure_kernel(const QualityArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned s_luma[QM_LDS_BYTES / 4];
  __shared__ long long s_part[QM_WAVES][5];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, SW = S >> 2;   // SW: words of a row
  const int R = min(max(*a.total, 0), a.cap);   // the classified ROIs, read where roi_resize and the classifier read them
  const int H = qm_strip_rows(S, QM_LDS_BYTES);   // Laplacian rows of a strip
  for (int r = blockIdx.x; r < R; r += gridDim.x) {
    const int b = a.roi_img[r], slot = a.roi_slot[r];
    if (b < 0 || b >= a.B || slot < 0 || slot >= a.max_det) continue;   // uniform: a record outside the call's frames is never written
    const u32x4* crop = reinterpret_cast<const u32x4*>(a.roi_rgb + (size_t)r * 3 * S * S);
    int s1 = 0;
    unsigned t1 = 0, t2 = 0, lo = 0, hi = 0;
    unsigned long long s2 = 0;
    int counted = 0;   // pixels [0, counted) are in the exposure sums already
    for (int y0 = 1; y0 <= S - 2; y0 += H) {
      const QmStrip strip = qm_strip(S, H, y0);
      const int p0 = strip.p0, p1 = strip.p1;   // the strip's pixels, both multiples of 16 (p1 rounded up to a whole unit)
      // ---- load: 16 pixels per thread and turn
      for (int u = (p0 >> 4) + tid; u < (p1 >> 4); u += QM_THREADS) {
        const u32x4 q0 = crop[3 * u], q1 = crop[3 * u + 1], q2 = crop[3 * u + 2];
        const unsigned w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
        unsigned y4[4];
        const bool count = (u << 4) >= counted;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // 4 pixels = 3 words -> one luma word
          unsigned packed = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int o = 12 * k + 3 * i;   // byte offset of the pixel in the unit
            const int Y = qm_luma(qm_byte(w[o >> 2], o & 3), qm_byte(w[(o + 1) >> 2], (o + 1) & 3), qm_byte(w[(o + 2) >> 2], (o + 2) & 3));
            packed |= (unsigned)Y << (8 * i);
            if (count) { t1 += Y; t2 += Y * Y; lo += Y <= LP_QM_CLIP_LO; hi += Y >= LP_QM_CLIP_HI; }
          }
          y4[k] = packed;
        }
        *reinterpret_cast<u32x4*>(&s_luma[((u << 4) - p0) >> 2]) = u32x4{y4[0], y4[1], y4[2], y4[3]};
      }
      counted = p1;
      __syncthreads();
      // ---- tap: the words of rows [y0, strip.y_end); every neighbour word lies inside the strip
      const int n_words = (strip.y_end - y0) * SW;
      for (int j = tid; j < n_words; j += QM_THREADS) {
        const int row = j / SW, xw = j - row * SW;
        const int k = (row + 1) * SW + xw;   // the word's index in the strip (row 0 of the strip is y0 - 1)
        const unsigned c = s_luma[k], up = s_luma[k - SW], dn = s_luma[k + SW], lf = s_luma[k - 1], rt = s_luma[k + 1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int x = 4 * xw + i;
          if (x >= 1 && x <= S - 2) {
            const int left = i > 0 ? qm_byte(c, i - 1) : qm_byte(lf, 3), right = i < 3 ? qm_byte(c, i + 1) : qm_byte(rt, 0);
            const int L = qm_laplacian(qm_byte(up, i), qm_byte(dn, i), left, right, qm_byte(c, i));
            s1 += L; s2 += (unsigned)(L * L);
          }
        }
      }
      __syncthreads();   // the strip is read before the next one replaces it
    }
    // ---- sums: wave, then workgroup
    const long long v[5] = {qm_wave_sum((long long)s1), qm_wave_sum((long long)s2), qm_wave_sum((long long)t1), qm_wave_sum((long long)t2),
                            qm_wave_sum((long long)lo | ((long long)hi << 32))};
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 5; ++i) s_part[wave][i] = v[i];
    }
    __syncthreads();
    if (tid == 0) {
      long long z[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int wv = 0; wv < QM_WAVES; ++wv)
#pragma unroll
        for (int i = 0; i < 5; ++i) z[i] += s_part[wv][i];
      QualitySums s;
      s.n = (int64_t)(S - 2) * (S - 2); s.s1 = z[0]; s.s2 = z[1];
      s.N = (int64_t)S * S; s.t1 = z[2]; s.t2 = z[3]; s.lo = z[4] & 0xFFFFFFFFll; s.hi = z[4] >> 32;
      QualityRec q;
      qm_record(s, &q);
      i32x4* o = reinterpret_cast<i32x4*>(a.out + (size_t)b * a.max_det + slot);
      o[0] = i32x4{__float_as_int(q.sharpness), __float_as_int(q.luma_mean), __float_as_int(q.luma_var), __float_as_int(q.clip_lo)};
      o[1] = i32x4{__float_as_int(q.clip_hi), q.flags, 0, 0};
    }
    __syncthreads();   // s_part is read before the next ROI's sums
  }
}

void launch_quality_clear(lp_quality* out, int n_records, hipStream_t st) {
  if (n_records <= 0) return;
  const int n_halves = n_records * 2;
  LP_LAUNCH(quality_clear_kernel, dim3((n_halves + 255) / 256), dim3(256), 0, st, reinterpret_cast<i32x4*>(out), n_halves);
  LP_HIP(hipGetLastError());
}

void launch_quality_measure(const QualityArgs& a, hipStream_t st) {
  LP_CHECK(a.S >= 4 && a.S <= LP_QM_S_MAX && a.S % 4 == 0 && a.B >= 1 && a.max_det >= 1, LP_ERR_ARG, "bad quality shape (crops of %d)", a.S);
  if (a.cap <= 0) return;
  LP_LAUNCH(quality_measure_kernel, dim3(std::min(a.cap, QM_MAX_GRID)), dim3(QM_THREADS), 0, st, a);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
