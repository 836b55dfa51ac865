// Mapped views (include/litepi.h "mapped views"): the three host functions of view_map.h's rules (lp_map_fixed, lp_map_render,
// lp_map_box: no handle, no device) and a handle's maps (lp_map_add, lp_map_clear).  The run calls are the views family's
// (views.cpp: lp_run_mapped*), the kernels map_kernels.hip's.
#include "handle.h"
#include "view_map.h"

namespace lp {

static void check_map_sizes(int S, int H, int W) {
  LP_CHECK(S >= 2 && S <= LP_MAP_SIDE_MAX, LP_ERR_ARG, "a map needs a view side of 2..%d (got %d)", LP_MAP_SIDE_MAX, S);
  LP_CHECK(H >= 1 && W >= 1 && H <= LP_MAP_SIDE_MAX && W <= LP_MAP_SIDE_MAX, LP_ERR_ARG, "a map needs a frame of 1..%d pixels a side (got %dx%d)",
           LP_MAP_SIDE_MAX, W, H);
}

// xy[S][S][2] -> fixed[S][S][2]; LP_ERR_ARG for a NaN
static void map_fixed(const float* xy, int S, int H, int W, int32_t* fixed) {
  for (long k = 0; k < (long)S * S; ++k)
    LP_CHECK(vm_fix(xy[2 * k], W, fixed + 2 * k) && vm_fix(xy[2 * k + 1], H, fixed + 2 * k + 1), LP_ERR_ARG,
             "map: NaN at view pixel (row %ld, column %ld)", k / S, k % S);
}

// the frame bytes a table's positions span: the bounding rectangle of its taps inside the frame, 3 bytes per pixel
static double map_footprint_bytes(const int32_t* fixed, int S, int H, int W) {
  int x0 = W, x1 = -1, y0 = H, y1 = -1;
  for (long k = 0; k < (long)S * S; ++k) {
    const int ix = fixed[2 * k] >> LP_MAP_FRAC_BITS, iy = fixed[2 * k + 1] >> LP_MAP_FRAC_BITS;
    x0 = std::min(x0, std::max(ix, 0)); x1 = std::max(x1, std::min(ix + 1, W - 1));
    y0 = std::min(y0, std::max(iy, 0)); y1 = std::max(y1, std::min(iy + 1, H - 1));
  }
  return x1 >= x0 && y1 >= y0 ? 3.0 * (x1 - x0 + 1) * (y1 - y0 + 1) : 0.0;
}

}  // namespace lp

using namespace lp;

extern "C" {

int lp_map_fixed(const float* xy, int S, int H, int W, int32_t* fixed) {
  LP_API_BEGIN
  LP_CHECK(xy && fixed, LP_ERR_ARG, "null argument");
  check_map_sizes(S, H, W);
  map_fixed(xy, S, H, W, fixed);
  LP_API_END
}

int lp_map_render(const int32_t* fixed, int S, const uint8_t* frame, int H, int W, uint8_t* out) {
  LP_API_BEGIN
  LP_CHECK(fixed && frame && out, LP_ERR_ARG, "null argument");
  check_map_sizes(S, H, W);
  for (long k = 0; k < (long)S * S; ++k) vm_pixel(frame, H, W, fixed[2 * k], fixed[2 * k + 1], out + 3 * k);
  LP_API_END
}

int lp_map_box(const int32_t* fixed, int S, int H, int W, const float* box, float* out) {
  LP_API_BEGIN
  LP_CHECK(fixed && box && out, LP_ERR_ARG, "null argument");
  check_map_sizes(S, H, W);
  vm_box(fixed, S, H, W, box, out);
  LP_API_END
}

int lp_map_add(lp_handle* h, const float* xy, int H, int W, int* id) {
  LP_API_BEGIN
  LP_CHECK(h && xy && id, LP_ERR_ARG, "null argument");
  check_square(h, "lp_map_add");
  const int S = h->cfg.det_input;
  check_map_sizes(S, H, W);
  LP_CHECK(S % 4 == 0, LP_ERR_STATE, "mapped views need det_input %% 4 == 0 (it is %d)", S);
  LP_CHECK((int)h->maps.size() < LP_MAP_MAX, LP_ERR_STATE, "the handle holds LP_MAP_MAX = %d maps: lp_map_clear first", LP_MAP_MAX);
  std::vector<int32_t> fixed((size_t)S * S * 2);
  map_fixed(xy, S, H, W, fixed.data());
  LP_HIP(hipSetDevice(h->cfg.device));
  auto m = std::make_unique<lp_handle::MapEntry>();
  m->fixed.alloc(fixed.size() * 4, false);
  LP_HIP(hipMemcpy(m->fixed.p, fixed.data(), fixed.size() * 4, hipMemcpyHostToDevice));
  m->H = H; m->W = W;
  m->foot_bytes = map_footprint_bytes(fixed.data(), S, H, W);
  *id = (int)h->maps.size();
  h->maps.push_back(std::move(m));
  LP_API_END
}

int lp_map_clear(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (!h->maps.empty()) {
    LP_HIP(hipSetDevice(h->cfg.device));
    LP_HIP(hipStreamSynchronize(h->stream));   // a step in flight may still read a table
    h->maps.clear();
  }
  h->tile_cache.clear();   // the call tables may name a freed map
  ++h->geom_ver;
  LP_API_END
}

}  // extern "C"
