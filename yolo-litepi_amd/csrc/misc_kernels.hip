// Byte-moving detector kernels: letterbox (front ends of letterbox_core.h), nearest upsample, SPPF pooling, add/copy.
// All HBM-bound: 16-byte vector accesses over NHWC channel groups, one thread per
// (pixel, 8-channel fp16 / 4-channel fp32 group).
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <cstdlib>

namespace lp {

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct VecT;
template <> struct VecT<half_t> { typedef half8 type; static constexpr int G = 8; };
template <> struct VecT<float> { typedef floatx4 type; static constexpr int G = 4; };

// ------------------------------------------------------------------------------------
// letterbox (reference e2e.py:66-86): front ends of the letterbox core (letterbox_core.h) over the whole images of the source
// buffer.  cv2.resize(INTER_LINEAR) on uint8 is restated there from OpenCV's published fixed-point algorithm; cv2 is absent
// from the build container: only the identity and pad-only cases are pinned.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void letterbox_kernel(const uint8_t* __restrict__ src, const ImgGeom* __restrict__ geom,
                                                        uint8_t* __restrict__ dst, int SH, int SW) {
  const int n = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= SH * SW) return;
  const ImgGeom gm = geom[n];
  lb_pixel_thread(lb_source(src, gm), lb_place(gm), dst + (long)n * SH * SW * 3, SW, idx);
}

// Tiled form: a workgroup owns an 8 x 128 tile of the letterboxed image and stages the two source rows of each of its output
// rows in LDS (cv2's non-antialiased INTER_LINEAR touches only those: at the 3.2x down-scale of a 2048 x 2048 frame 5/8 of the
// source rows).  HBM: every needed source byte once, in >= 1 KB runs; the per-pixel kernel gathers 12 single bytes per pixel.
// The 16-byte loads are aligned by the address and bounded by the image itself, whatever the caller's buffer holds around it.
__global__ __launch_bounds__(256) void letterbox_tiled_kernel(const uint8_t* __restrict__ src, const ImgGeom* __restrict__ geom,
                                                              uint8_t* __restrict__ dst, int SH, int SW, int row_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t band[];   // [2 * LB_TH][row_cap]
  __shared__ int s_shift[2 * LB_TH];                                // byte index of source byte b0 inside an LDS row
  const int n = blockIdx.z;
  const ImgGeom gm = geom[n];
  lb_tile(lb_source(src, gm), lb_place(gm), dst + (long)n * SH * SW * 3, SH, SW, band, row_cap, s_shift);
}

// host_geoms (optional, the B geometries): lets the launcher size the tiled kernel's LDS rows; without them, or when the rows
// do not fit, the per-pixel kernel runs
void launch_letterbox(const uint8_t* src, const ImgGeom* geom, uint8_t* dst, int B, int SH, int SW, hipStream_t st,
                      const ImgGeom* host_geoms) {
  static const bool no_tiled = getenv("LITEPI_LB_NAIVE") != nullptr;   // A/B switch
  if (host_geoms && !no_tiled && SW % 4 == 0) {
    int cap = 0;
    for (int i = 0; i < B; ++i) cap = std::max(cap, lb_row_cap(host_geoms[i].w, host_geoms[i].new_w, LB_TW));
    if (lb_rows_fit(cap)) {
      dim3 grid(ceil_div(SW, LB_TW), ceil_div(SH, LB_TH), B);
      LP_LAUNCH(letterbox_tiled_kernel, grid, dim3(256), (size_t)cap * 2 * LB_TH, st, src, geom, dst, SH, SW, cap);
      LP_HIP(hipGetLastError());
      return;
    }
  }
  dim3 grid(ceil_div(SH * SW, 256), B);
  LP_LAUNCH(letterbox_kernel, grid, dim3(256), 0, st, src, geom, dst, SH, SW);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void upsample2x_kernel(const T* __restrict__ in, T* __restrict__ out, int N, int H, int W,
                                                         int CG, int in_pitch, int out_pitch) {
  constexpr int G = VecT<T>::G;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)N * (2 * H) * (2 * W) * CG;
  if (idx >= total) return;
  const int cg = (int)(idx % CG);
  const long pix = idx / CG;
  const int ox = (int)(pix % (2 * W));
  const int oy = (int)((pix / (2 * W)) % (2 * H));
  const int n = (int)(pix / ((long)4 * W * H));
  const u32x4 v = *reinterpret_cast<const u32x4*>(in + ((long)(n * H + (oy >> 1)) * W + (ox >> 1)) * in_pitch + cg * G);
  *reinterpret_cast<u32x4*>(out + pix * out_pitch + cg * G) = v;
}

void launch_upsample2x(int prec, const View& in, const View& out, int N, hipStream_t st) {
  LP_CHECK(out.H == 2 * in.H && out.W == 2 * in.W && out.C >= in.C, LP_ERR_STATE, "upsample2x: shape mismatch");
  const int G = prec == LP_FP16 ? 8 : 4;
  const int CG = in.C / G;
  const long total = (long)N * out.H * out.W * CG;
  dim3 grid((unsigned)((total + 255) / 256));
  if (prec == LP_FP16)
    LP_LAUNCH(upsample2x_kernel<half_t>, grid, dim3(256), 0, st, (const half_t*)in.base, (half_t*)out.base, N, in.H,
                       in.W, CG, in.pitch, out.pitch);
  else
    LP_LAUNCH(upsample2x_kernel<float>, grid, dim3(256), 0, st, (const float*)in.base, (float*)out.base, N, in.H,
                       in.W, CG, in.pitch, out.pitch);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// SPPF: y1 = pool5(x), y2 = pool5(y1), y3 = pool5(y2) with -inf padding == max over the
// clipped 5x5 / 9x9 / 13x13 windows of x.
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void sppf_pool_kernel(const T* __restrict__ in, T* __restrict__ o1, T* __restrict__ o2,
                                                        T* __restrict__ o3, int N, int H, int W, int CG, int in_pitch,
                                                        int p1, int p2, int p3) {
  typedef typename VecT<T>::type vec;
  constexpr int G = VecT<T>::G;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)N * H * W * CG;
  if (idx >= total) return;
  const int cg = (int)(idx % CG);
  const long pix = idx / CG;
  const int x = (int)(pix % W);
  const int y = (int)((pix / W) % H);
  const int n = (int)(pix / ((long)W * H));
  vec m5, m9, m13;
#pragma unroll
  for (int i = 0; i < G; ++i) { m5[i] = (T)-INFINITY; m9[i] = (T)-INFINITY; m13[i] = (T)-INFINITY; }
  for (int dy = -6; dy <= 6; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    const int ady = dy < 0 ? -dy : dy;
    for (int dx = -6; dx <= 6; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= W) continue;
      const int adx = dx < 0 ? -dx : dx;
      const int r = ady > adx ? ady : adx;
      const vec v = *reinterpret_cast<const vec*>(in + ((long)(n * H + yy) * W + xx) * in_pitch + cg * G);
#pragma unroll
      for (int i = 0; i < G; ++i) {
        m13[i] = v[i] > m13[i] ? v[i] : m13[i];
        if (r <= 4) m9[i] = v[i] > m9[i] ? v[i] : m9[i];
        if (r <= 2) m5[i] = v[i] > m5[i] ? v[i] : m5[i];
      }
    }
  }
  *reinterpret_cast<vec*>(o1 + pix * p1 + cg * G) = m5;
  *reinterpret_cast<vec*>(o2 + pix * p2 + cg * G) = m9;
  *reinterpret_cast<vec*>(o3 + pix * p3 + cg * G) = m13;
}

// LDS version for maps up to 40x40: one workgroup per (image, 16-byte channel group); each 5x5
// pool is separable (row max, then column max), cascaded three times in place.
#define SPPF_MAX_PIX 1600
template <typename T>
__global__ __launch_bounds__(256) void sppf_pool_lds_kernel(const T* __restrict__ in, T* __restrict__ o1, T* __restrict__ o2,
                                                            T* __restrict__ o3, int H, int W, int CG, int in_pitch, int p1,
                                                            int p2, int p3) {
  typedef typename VecT<T>::type vec;
  constexpr int G = VecT<T>::G;
  __shared__ vec A[SPPF_MAX_PIX];
  __shared__ vec B[SPPF_MAX_PIX];
  const int cg = blockIdx.x % CG, n = blockIdx.x / CG;
  const int HW = H * W, tid = threadIdx.x;
  const long base = (long)n * HW;
  for (int p = tid; p < HW; p += 256) A[p] = *reinterpret_cast<const vec*>(in + (base + p) * in_pitch + cg * G);
  __syncthreads();
  T* outs[3] = {o1, o2, o3};
  const int pitches[3] = {p1, p2, p3};
  for (int stage = 0; stage < 3; ++stage) {
    for (int p = tid; p < HW; p += 256) {
      const int y = p / W, x = p - y * W;
      vec m = A[p];
      for (int d = -2; d <= 2; ++d) {
        const int xx = x + d;
        if (d == 0 || xx < 0 || xx >= W) continue;
        const vec v = A[y * W + xx];
#pragma unroll
        for (int i = 0; i < G; ++i) m[i] = v[i] > m[i] ? v[i] : m[i];
      }
      B[p] = m;
    }
    __syncthreads();
    for (int p = tid; p < HW; p += 256) {
      const int y = p / W, x = p - y * W;
      vec m = B[p];
      for (int d = -2; d <= 2; ++d) {
        const int yy = y + d;
        if (d == 0 || yy < 0 || yy >= H) continue;
        const vec v = B[yy * W + x];
#pragma unroll
        for (int i = 0; i < G; ++i) m[i] = v[i] > m[i] ? v[i] : m[i];
      }
      A[p] = m;
      *reinterpret_cast<vec*>(outs[stage] + (base + p) * pitches[stage] + cg * G) = m;
    }
    __syncthreads();
  }
}

void launch_sppf_pool(int prec, const View& in, const View& o1, const View& o2, const View& o3, int N, hipStream_t st) {
  const int G = prec == LP_FP16 ? 8 : 4;
  const int CG = in.C / G;
  if (in.H * in.W <= SPPF_MAX_PIX) {
    dim3 grid((unsigned)(N * CG));
    if (prec == LP_FP16)
      LP_LAUNCH(sppf_pool_lds_kernel<half_t>, grid, dim3(256), 0, st, (const half_t*)in.base, (half_t*)o1.base,
                         (half_t*)o2.base, (half_t*)o3.base, in.H, in.W, CG, in.pitch, o1.pitch, o2.pitch, o3.pitch);
    else
      LP_LAUNCH(sppf_pool_lds_kernel<float>, grid, dim3(256), 0, st, (const float*)in.base, (float*)o1.base,
                         (float*)o2.base, (float*)o3.base, in.H, in.W, CG, in.pitch, o1.pitch, o2.pitch, o3.pitch);
    LP_HIP(hipGetLastError());
    return;
  }
  const long total = (long)N * in.H * in.W * CG;
  dim3 grid((unsigned)((total + 255) / 256));
  if (prec == LP_FP16)
    LP_LAUNCH(sppf_pool_kernel<half_t>, grid, dim3(256), 0, st, (const half_t*)in.base, (half_t*)o1.base,
                       (half_t*)o2.base, (half_t*)o3.base, N, in.H, in.W, CG, in.pitch, o1.pitch, o2.pitch, o3.pitch);
  else
    LP_LAUNCH(sppf_pool_kernel<float>, grid, dim3(256), 0, st, (const float*)in.base, (float*)o1.base,
                       (float*)o2.base, (float*)o3.base, N, in.H, in.W, CG, in.pitch, o1.pitch, o2.pitch, o3.pitch);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void eltwise_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out,
                                                      long npix, int CG, int pa, int pb, int po) {
  typedef typename VecT<T>::type vec;
  constexpr int G = VecT<T>::G;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npix * CG) return;
  const int cg = (int)(idx % CG);
  const long pix = idx / CG;
  vec v = *reinterpret_cast<const vec*>(a + pix * pa + cg * G);
  if (ADD) {
    const vec w = *reinterpret_cast<const vec*>(b + pix * pb + cg * G);
#pragma unroll
    for (int i = 0; i < G; ++i) v[i] = (T)((float)v[i] + (float)w[i]);
  }
  *reinterpret_cast<vec*>(out + pix * po + cg * G) = v;
}

void launch_add(int prec, const View& a, const View& b, const View& out, int N, hipStream_t st) {
  const int G = prec == LP_FP16 ? 8 : 4;
  const int CG = a.C / G;
  const long npix = (long)N * a.H * a.W;
  dim3 grid((unsigned)((npix * CG + 255) / 256));
  if (prec == LP_FP16)
    LP_LAUNCH((eltwise_kernel<half_t, true>), grid, dim3(256), 0, st, (const half_t*)a.base, (const half_t*)b.base,
                       (half_t*)out.base, npix, CG, a.pitch, b.pitch, out.pitch);
  else
    LP_LAUNCH((eltwise_kernel<float, true>), grid, dim3(256), 0, st, (const float*)a.base, (const float*)b.base,
                       (float*)out.base, npix, CG, a.pitch, b.pitch, out.pitch);
  LP_HIP(hipGetLastError());
}

void launch_copy(int prec, const View& in, const View& out, int N, hipStream_t st) {
  const int G = prec == LP_FP16 ? 8 : 4;
  const int CG = in.C / G;
  const long npix = (long)N * in.H * in.W;
  dim3 grid((unsigned)((npix * CG + 255) / 256));
  if (prec == LP_FP16)
    LP_LAUNCH((eltwise_kernel<half_t, false>), grid, dim3(256), 0, st, (const half_t*)in.base, (const half_t*)nullptr,
                       (half_t*)out.base, npix, CG, in.pitch, 0, out.pitch);
  else
    LP_LAUNCH((eltwise_kernel<float, false>), grid, dim3(256), 0, st, (const float*)in.base, (const float*)nullptr,
                       (float*)out.base, npix, CG, in.pitch, 0, out.pitch);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// Depthwise 3x3 / stride 1 / pad 1 (+bias, optional SiLU) on a detector activation (NHWC).  YOLO11's DWConv layers
// (Detect class branch) -- ConvolutionDepthWise in the NCNN export.  w: fp32 [9][C] over physical channels.
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_act_kernel(const T* __restrict__ in, T* __restrict__ out,
                                                            const float* __restrict__ w, const float* __restrict__ bias,
                                                            long npix, int H, int W, int C, int in_pitch, int out_pitch, int act) {
  typedef typename VecT<T>::type vec;
  constexpr int G = VecT<T>::G;
  const int CG = C / G;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= npix * CG) return;
  const int cg = (int)(idx % CG);
  const long pix = idx / CG;
  const int ox = (int)(pix % W), oy = (int)((pix / W) % H);
  float acc[G];
#pragma unroll
  for (int i = 0; i < G; ++i) acc[i] = bias[cg * G + i];
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = oy - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = ox - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      const vec v = *reinterpret_cast<const vec*>(in + (pix + (long)(ky - 1) * W + (kx - 1)) * in_pitch + cg * G);
      const float* wr = w + (ky * 3 + kx) * C + cg * G;
#pragma unroll
      for (int i = 0; i < G; ++i) acc[i] = fmaf((float)v[i], wr[i], acc[i]);
    }
  }
  vec o;
#pragma unroll
  for (int i = 0; i < G; ++i) o[i] = (T)(act == ACT_SILU ? acc[i] * __builtin_amdgcn_rcpf(1.f + __expf(-acc[i])) : acc[i]);
  *reinterpret_cast<vec*>(out + pix * out_pitch + cg * G) = o;
}

void launch_dwconv3x3_act(int prec, const View& in, const View& out, const float* w, const float* bias, int act, int N, hipStream_t st) {
  const int G = prec == LP_FP16 ? 8 : 4;
  LP_CHECK(in.C == out.C && in.C % G == 0 && in.H == out.H && in.W == out.W, LP_ERR_STATE, "dwconv3x3: view mismatch");
  const long npix = (long)N * in.H * in.W;
  dim3 grid((unsigned)((npix * (in.C / G) + 255) / 256));
  if (prec == LP_FP16)
    LP_LAUNCH(dwconv3x3_act_kernel<half_t>, grid, dim3(256), 0, st, (const half_t*)in.base, (half_t*)out.base, w, bias, npix,
                       in.H, in.W, in.C, in.pitch, out.pitch, act);
  else
    LP_LAUNCH(dwconv3x3_act_kernel<float>, grid, dim3(256), 0, st, (const float*)in.base, (float*)out.base, w, bias, npix,
                       in.H, in.W, in.C, in.pitch, out.pitch, act);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// YOLO11 C2PSA attention (model.ncnn.param of the reference's yolo11 export, layers reshape_166 .. add_7): the qkv
// tensor [N, HW, heads*(2*dk+dv)] holds per head dk query, dk key and dv value channels.  Per head:
//     P = softmax_m(scale * q_n . k_m),   o_n = sum_m P[n][m] v_m,   out = o + dwconv3x3(v) + pe_bias
// One workgroup = 16 queries of one (image, head); scores in LDS (fp32), K / V read through L2 (a head's K and V are
// ~75 KB).  fp32 arithmetic whatever the storage type.
// ------------------------------------------------------------------------------------
#define ATT_QB 16
template <typename T>
__global__ __launch_bounds__(256) void psa_attention_kernel(const T* __restrict__ qkv, T* __restrict__ out, const float* __restrict__ pe_w,
                                                            const float* __restrict__ pe_b, int H, int W, int heads, int dk, int dv,
                                                            float scale, int in_pitch, int out_pitch) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int HW = H * W;
  float* sq = reinterpret_cast<float*>(smem);         // [ATT_QB][dk]
  float* ss = sq + ATT_QB * dk;                        // [ATT_QB][HW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x, h = blockIdx.y, n0 = blockIdx.z * ATT_QB;
  const int hc = h * (2 * dk + dv);
  const T* base = qkv + (long)n * HW * in_pitch + hc;
  for (int i = tid; i < ATT_QB * dk; i += 256) {
    const int qi = i / dk, j = i - qi * dk;
    sq[i] = n0 + qi < HW ? (float)base[(long)(n0 + qi) * in_pitch + j] : 0.f;
  }
  __syncthreads();
  for (int m = tid; m < HW; m += 256) {
    float acc[ATT_QB];
#pragma unroll
    for (int qi = 0; qi < ATT_QB; ++qi) acc[qi] = 0.f;
    const T* kp = base + (long)m * in_pitch + dk;
    for (int j = 0; j < dk; ++j) {
      const float kv = (float)kp[j];
#pragma unroll
      for (int qi = 0; qi < ATT_QB; ++qi) acc[qi] = fmaf(sq[qi * dk + j], kv, acc[qi]);
    }
#pragma unroll
    for (int qi = 0; qi < ATT_QB; ++qi) ss[qi * HW + m] = acc[qi] * scale;
  }
  __syncthreads();
  for (int qi = wave; qi < ATT_QB; qi += 4) {  // softmax over the keys, one wave per query row
    float mx = -3.0e38f;
    for (int m = lane; m < HW; m += 64) mx = fmaxf(mx, ss[qi * HW + m]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int m = lane; m < HW; m += 64) { const float e = expf(ss[qi * HW + m] - mx); ss[qi * HW + m] = e; sum += e; }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.f / sum;
    for (int m = lane; m < HW; m += 64) ss[qi * HW + m] *= inv;
  }
  __syncthreads();
  for (int i = tid; i < ATT_QB * dv; i += 256) {
    const int qi = i / dv, d = i - qi * dv;
    const int q = n0 + qi;
    if (q >= HW) continue;
    const T* vp = base + 2 * dk + d;
    float acc = 0.f;
    for (int m = 0; m < HW; ++m) acc = fmaf(ss[qi * HW + m], (float)vp[(long)m * in_pitch], acc);
    // positional encoding: depthwise 3x3 over the value map of this channel
    const int c = h * dv + d, oy = q / W, ox = q - oy * W;
    float pe = pe_b[c];
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy - 1 + ky;
      if (iy < 0 || iy >= H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox - 1 + kx;
        if (ix < 0 || ix >= W) continue;
        pe = fmaf((float)vp[(long)(iy * W + ix) * in_pitch], pe_w[(ky * 3 + kx) * heads * dv + c], pe);
      }
    }
    out[((long)n * HW + q) * out_pitch + c] = (T)(acc + pe);
  }
}

void launch_psa_attention(int prec, const View& qkv, const View& out, const float* pe_w, const float* pe_b, int heads, int dk, int dv,
                          float scale, int N, hipStream_t st) {
  const int HW = qkv.H * qkv.W;
  LP_CHECK(qkv.C >= heads * (2 * dk + dv) && out.C >= heads * dv && out.H == qkv.H && out.W == qkv.W, LP_ERR_STATE, "attention: view mismatch");
  const size_t lds = (size_t)ATT_QB * (dk + HW) * 4;
  LP_CHECK(lds <= 150 * 1024, LP_ERR_GRAPH, "attention over %d positions does not fit LDS", HW);
  dim3 grid(N, heads, (HW + ATT_QB - 1) / ATT_QB);
  if (prec == LP_FP16) {
    set_max_dynamic_lds(reinterpret_cast<const void*>(psa_attention_kernel<half_t>), 160 * 1024);
    LP_LAUNCH(psa_attention_kernel<half_t>, grid, dim3(256), lds, st, (const half_t*)qkv.base, (half_t*)out.base, pe_w, pe_b, qkv.H,
                       qkv.W, heads, dk, dv, scale, qkv.pitch, out.pitch);
  } else {
    set_max_dynamic_lds(reinterpret_cast<const void*>(psa_attention_kernel<float>), 160 * 1024);
    LP_LAUNCH(psa_attention_kernel<float>, grid, dim3(256), lds, st, (const float*)qkv.base, (float*)out.base, pe_w, pe_b, qkv.H,
                       qkv.W, heads, dk, dv, scale, qkv.pitch, out.pitch);
  }
  LP_HIP(hipGetLastError());
}

}  // namespace lp
