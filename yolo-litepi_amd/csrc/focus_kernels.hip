// Focus views (the rule is stated in include/litepi.h, lp_focus_config): per frame, the windows the tracker's
// state asks for and the sweep over the window grid, chosen on the device and written straight into the view tables the
// gather, the decode and the frame NMS of a captured step read.  Like the tracker's kernel this is a latency chain per
// camera, not a throughput kernel: ONE WORKGROUP per stream present in the call.  Thread t owns table slot t (T <= 256): it
// predicts and clips its track and finds its place among the askers with a counting rank over LDS.  The placement is serial
// over the askers (each placed window removes later askers) and parallel over the placed windows: wave 0 walks the ranked
// askers, lane k holds window k (slots <= 16) and a ballot says whether any window covers the asker.  The sweep and the table
// entries -- the ViewWin and the ImgGeom of every slot, in fp64 with every operation rounded on its own so that they equal the
// host's make_geom / window_geom bit for bit -- are written by the lanes of wave 0, one slot each.
#include "common.h"
#include "kernels.h"

namespace lp {

#define FOCUS_THREADS 256   // lp_track_config::max_tracks <= 256
#define FOCUS_MAX_SLOTS 16

// one axis of lp_view_grid: n windows of side min(L, tile); origin of window k
__device__ __forceinline__ int grid_count(int L, int tile, int step) { return L <= tile ? 1 : 1 + (L - tile + step - 1) / step; }
__device__ __forceinline__ int grid_origin(int L, int tile, int step, int k) { return L <= tile ? 0 : min(k * step, L - tile); }

// make_geom of a wh x ww image for det_input S, in doubles (pipeline.cpp), pads moved by the window's origin (views.cpp window_geom)
__device__ __forceinline__ void window_geometry(int x, int y, int ww, int wh, int S, int& new_w, int& new_h, int& top, int& left, float& ratio,
                                                float& pad_w, float& pad_h) {
  const double r = fmin(__ddiv_rn((double)S, (double)wh), __ddiv_rn((double)S, (double)ww));
  new_w = (int)rint(__dmul_rn((double)ww, r));
  new_h = (int)rint(__dmul_rn((double)wh, r));
  const double dw = __ddiv_rn((double)(S - new_w), 2.0), dh = __ddiv_rn((double)(S - new_h), 2.0);
  top = (int)rint(__dsub_rn(dh, 0.1));
  left = (int)rint(__dsub_rn(dw, 0.1));
  ratio = (float)r;
  pad_w = (float)__dsub_rn(dw, __dmul_rn(r, (double)x));
  pad_h = (float)__dsub_rn(dh, __dmul_rn(r, (double)y));
}

__global__ __launch_bounds__(FOCUS_THREADS) void focus_plan_kernel(const FocusArgs a) {
  __shared__ float s_box[4][FOCUS_THREADS];
  __shared__ int s_hits[FOCUS_THREADS], s_ask[FOCUS_THREADS], s_order[FOCUS_THREADS];
  const int tid = threadIdx.x, lane = tid & 63;
  const TrackJob job = a.jobs[blockIdx.x];
  const int* frames = a.frames + job.first;
  const int T = a.T, slots = a.slots;

  // the stream's track, one slot per thread: fixed for the call
  float box[4] = {0.f, 0.f, 0.f, 0.f}, vel[4] = {0.f, 0.f, 0.f, 0.f};
  int hits = 0, missed = 0;
  bool live = false;
  if (tid < T) {
    const TrackSlot q = a.table[(size_t)job.stream * T + tid];
#pragma unroll
    for (int k = 0; k < 4; ++k) { box[k] = q.box[k]; vel[k] = q.vel[k]; }
    hits = q.hits; missed = q.missed; live = q.live != 0;
  }
  int cursor = a.state[job.stream].cursor, unserved = a.state[job.stream].unserved;

  for (int j = 0; j < job.nframes; ++j) {
    const int b = frames[j];
    const int H = a.fh[b], W = a.fw[b];
    const float rf = a.frf[b];
    // ---- 1 ask
    bool ask = false;
    float c[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      const float dt = (float)(missed + 1 + j);
      float p[4];
      bool nan = false;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        p[k] = a.motion ? __fadd_rn(box[k], __fmul_rn(vel[k], dt)) : box[k];
        nan = nan || p[k] != p[k];
      }
      c[0] = fmaxf(p[0], 0.f); c[1] = fmaxf(p[1], 0.f); c[2] = fminf(p[2], (float)W); c[3] = fminf(p[3], (float)H);
      const float bw = __fsub_rn(c[2], c[0]), bh = __fsub_rn(c[3], c[1]);
      ask = !nan && bw > 0.f && bh > 0.f && __fmul_rn(fmaxf(bw, bh), rf) < a.small_px;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s_box[k][tid] = c[k];
    s_hits[tid] = hits;
    s_ask[tid] = ask ? 1 : 0;
    __syncthreads();
    // ---- the askers' order: hits descending, ties to the lower slot (a counting rank: every asker counts those before it)
    if (ask) {
      int rank = 0;
      for (int u = 0; u < T; ++u) rank += (s_ask[u] && (s_hits[u] > hits || (s_hits[u] == hits && u < tid))) ? 1 : 0;
      s_order[rank] = tid;
    }
    const int n_ask = __syncthreads_count(ask ? 1 : 0);

    if (tid < 64) {   // wave 0; everything below is wave-uniform except the window a lane holds
      // ---- 2 place
      int wx = 0, wy = 0, ww = 0, wh = 0, np = 0;
      for (int i = 0; i < n_ask; ++i) {
        const int s = s_order[i];
        const float x1 = s_box[0][s], y1 = s_box[1][s], x2 = s_box[2][s], y2 = s_box[3][s];
        const bool cov = lane < np && (wx == 0 || x1 >= (float)((long long)wx + a.border)) &&
                         (wx + ww == W || x2 <= (float)((long long)wx + ww - a.border)) &&
                         (wy == 0 || y1 >= (float)((long long)wy + a.border)) && (wy + wh == H || y2 <= (float)((long long)wy + wh - a.border));
        if (__ballot(cov) != 0ull) continue;
        if (np >= slots) { ++unserved; continue; }
        const float want = ceilf(__fmul_rn(a.margin, fmaxf(__fsub_rn(x2, x1), __fsub_rn(y2, y1))));
        const int side = want >= (float)a.side_max ? a.side_max : (want <= (float)a.side_min ? a.side_min : (int)want);
        const int pw = min(side, W), ph = min(side, H);
        const int cx = (int)floorf(__fmul_rn(__fadd_rn(x1, x2), 0.5f)), cy = (int)floorf(__fmul_rn(__fadd_rn(y1, y2), 0.5f));
        if (lane == np) {
          wx = min(max(cx - pw / 2, 0), W - pw); wy = min(max(cy - ph / 2, 0), H - ph);
          ww = pw; wh = ph;
        }
        ++np;
      }
      // ---- 3 sweep
      if (a.sweep) {
        const int step = a.side_min - a.sweep_overlap;
        const int nx = grid_count(W, a.side_min, step), ny = grid_count(H, a.side_min, step), n = nx * ny;
        if (n > 1) {
          const int r = min(slots - np, n);
          if (lane >= np && lane < np + r) {
            const int g = (cursor + (lane - np)) % n;
            wx = grid_origin(W, a.side_min, step, g % nx); wy = grid_origin(H, a.side_min, step, g / nx);
            ww = min(W, a.side_min); wh = min(H, a.side_min);
          }
          cursor = (cursor + r) % n;
          np += r;
        }
      }
      // ---- 4 the slots: windows, then empty ones
      if (lane < slots) {
        const bool empty = lane >= np;
        if (empty) { wx = 0; wy = 0; ww = 0; wh = 0; }
        if (a.views) {
          int* v = a.views + ((size_t)b * slots + lane) * 4;
          v[0] = wx; v[1] = wy; v[2] = ww; v[3] = wh;
        }
        if (a.vwin) {
          const ImgGeom fg = a.fgeom[b];
          ImgGeom g = fg;   // an empty slot keeps the whole frame's geometry: its view is all bars, its candidates are dropped
          ViewWin w;
          w.src_off = fg.src_off; w.pitch = 3 * fg.w; w.frame_bytes = (long)fg.h * w.pitch;
          w.x = wx; w.y = wy; w.w = ww; w.h = wh;
          w.new_w = 0; w.new_h = 0; w.top = 0; w.left = 0; w.pad = 0;
          if (!empty) {
            window_geometry(wx, wy, ww, wh, a.S, g.new_w, g.new_h, g.top, g.left, g.ratio, g.pad_w, g.pad_h);
            w.new_w = g.new_w; w.new_h = g.new_h; w.top = g.top; w.left = g.left;
          }
          const int slot = a.B + b * slots + lane;
          a.vwin[b * slots + lane] = w;
          // field by field: the entry's padding bytes stay as the host's upload left them
          ImgGeom* o = a.geom + slot;
          o->src_off = g.src_off; o->h = g.h; o->w = g.w; o->new_w = g.new_w; o->new_h = g.new_h; o->top = g.top; o->left = g.left;
          o->ratio = g.ratio; o->pad_w = g.pad_w; o->pad_h = g.pad_h;
          a.dead[slot] = empty ? 1 : 0;
          if (lane == 0) a.dead[b] = 0;   // the whole-frame view
        }
      }
    }
    __syncthreads();   // the next frame overwrites the LDS arrays
  }
  if (tid == 0 && a.advance) {
    a.state[job.stream].cursor = cursor;
    a.state[job.stream].unserved = unserved;
  }
}

void launch_focus_plan(const FocusArgs& a, int n_jobs, hipStream_t st) {
  if (n_jobs <= 0) return;
  LP_CHECK(a.T >= 1 && a.T <= FOCUS_THREADS && a.slots >= 1 && a.slots <= FOCUS_MAX_SLOTS, LP_ERR_ARG, "focus plan: %d tracks, %d slots", a.T,
           a.slots);
  LP_LAUNCH(focus_plan_kernel, dim3(n_jobs), dim3(FOCUS_THREADS), 0, st, a);
  LP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void focus_mask_kernel(const int* __restrict__ dead, int* __restrict__ cand_count, int V) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < V && dead[v]) cand_count[v] = 0;
}

void launch_focus_mask(const int* dead, int* cand_count, int V, hipStream_t st) {
  if (V <= 0) return;
  LP_LAUNCH(focus_mask_kernel, dim3(ceil_div(V, 256)), dim3(256), 0, st, dead, cand_count, V);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
