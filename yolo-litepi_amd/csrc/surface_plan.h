// Decoder surfaces (include/litepi.h lp_surface): the argument rules and the converter's per-frame record
// (the slot policy of its pinned ring is ring_slots.h).  Host-pure (no HIP headers): tests/native/surface_plan_check.cpp builds
// on the two headers alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

#include "error.h"

namespace lp {

// One decoder surface of a conversion call, device resident, 48 bytes: absolute plane addresses and a pitch per plane, so the
// table is the only thing that changes between calls on rotating surfaces.
struct SurfFrame {
  const uint8_t* y;      // first luma byte
  const uint8_t* uv;     // first byte of the interleaved chroma rows
  long dst_off;          // byte offset of the BGR frame in the destination buffer (ImgGeom::src_off of the same frame)
  int h, w;              // even luma size in pixels
  int pitch_y, pitch_uv; // bytes per row of each plane, the zeros resolved
  int aligned;           // 1: every 16-byte access of the frame's full blocks is 16-byte aligned
  int pad;
};
static_assert(sizeof(SurfFrame) == 48, "the device table's record");

inline int surface_sample_bytes(int pixfmt) { return pixfmt == LP_SURF_P010 ? 2 : 1; }

// the rules of include/litepi.h that need no handle; same_size: every surface as large as the first (the views variant)
inline void check_surfaces(const lp_surface_format* fmt, const lp_surface* s, int B, bool same_size) {
  LP_CHECK(fmt && s, LP_ERR_ARG, "null surface format or surface array");
  LP_CHECK(fmt->pixfmt == LP_SURF_NV12 || fmt->pixfmt == LP_SURF_P010, LP_ERR_ARG, "unknown surface pixel format %d", fmt->pixfmt);
  LP_CHECK(fmt->matrix == LP_CSC_BT601_LIMITED || fmt->matrix == LP_CSC_BT709_LIMITED, LP_ERR_ARG, "unknown colour matrix %d", fmt->matrix);
  for (int r : fmt->reserved) LP_CHECK(r == 0, LP_ERR_ARG, "lp_surface_format: reserved words must be zero");
  LP_CHECK(B >= 1, LP_ERR_ARG, "%d surfaces", B);
  const int bps = surface_sample_bytes(fmt->pixfmt);
  for (int i = 0; i < B; ++i) {
    const lp_surface& f = s[i];
    for (int r : f.reserved) LP_CHECK(r == 0, LP_ERR_ARG, "surface %d: reserved words must be zero", i);
    LP_CHECK(f.plane[0] && f.plane[1], LP_ERR_ARG, "surface %d: null plane", i);
    LP_CHECK(f.height > 0 && f.width > 0 && f.height % 2 == 0 && f.width % 2 == 0, LP_ERR_ARG,
             "surface %d: a %dx%d frame; width and height must be even and positive", i, f.width, f.height);
    const int64_t row = (int64_t)bps * f.width;
    LP_CHECK(row <= INT32_MAX, LP_ERR_ARG, "surface %d: a row of %lld bytes", i, (long long)row);
    for (int p = 0; p < 2; ++p) {
      LP_CHECK(f.pitch[p] >= 0, LP_ERR_ARG, "surface %d: negative pitch %d of plane %d", i, f.pitch[p], p);
      LP_CHECK(f.pitch[p] == 0 || f.pitch[p] >= row, LP_ERR_ARG, "surface %d: pitch %d of plane %d is below the row's %lld bytes", i, f.pitch[p],
               p, (long long)row);
      if (bps == 2)
        LP_CHECK(reinterpret_cast<uintptr_t>(f.plane[p]) % 2 == 0 && f.pitch[p] % 2 == 0, LP_ERR_ARG,
                 "surface %d: P010 plane %d needs an even address and an even pitch", i, p);
    }
    LP_CHECK(!same_size || (f.height == s[0].height && f.width == s[0].width), LP_ERR_ARG,
             "surface %d is %dx%d, surface 0 is %dx%d: this entry point takes surfaces of one size", i, f.width, f.height, s[0].width,
             s[0].height);
  }
}

// the records of B checked surfaces whose BGR frames go to dst + dst_off[i]; returns the launch's max_blocks (the largest
// (h / 2) * ceil(w / 16) of the table)
inline int fill_surface_table(const lp_surface_format& fmt, const lp_surface* s, int B, const void* dst, const long* dst_off, SurfFrame* out) {
  const int bps = surface_sample_bytes(fmt.pixfmt);
  int max_blocks = 0;
  for (int i = 0; i < B; ++i) {
    SurfFrame f;
    memset(&f, 0, sizeof(f));
    f.y = static_cast<const uint8_t*>(s[i].plane[0]); f.uv = static_cast<const uint8_t*>(s[i].plane[1]);
    f.dst_off = dst_off[i]; f.h = s[i].height; f.w = s[i].width;
    f.pitch_y = s[i].pitch[0] ? s[i].pitch[0] : bps * f.w;
    f.pitch_uv = s[i].pitch[1] ? s[i].pitch[1] : bps * f.w;
    f.aligned = reinterpret_cast<uintptr_t>(f.y) % 16 == 0 && reinterpret_cast<uintptr_t>(f.uv) % 16 == 0 && f.pitch_y % 16 == 0 &&
                f.pitch_uv % 16 == 0 && f.w % 16 == 0 && (reinterpret_cast<uintptr_t>(dst) + f.dst_off) % 16 == 0;
    out[i] = f;
    max_blocks = std::max(max_blocks, (f.h / 2) * ((f.w + 15) / 16));
  }
  return max_blocks;
}

}  // namespace lp
