// Stand-alone check of csrc/view_map.h (the table, pixel and box rules of mapped views, shared by lp_map_fixed / lp_map_render /
// lp_map_box and the device kernels), built with -fsanitize=address,undefined by tests/test_mapped_cpu.py.  Every frame is a
// heap block of exactly H * W * 3 bytes and every table one of exactly S * S * 2 ints, so a tap or a table read one byte
// outside is reported by the sanitizer.  It renders random tables (positions uniform in [-3, L + 2]) and extreme ones (huge,
// infinite, the frame's corners, its last pixel with zero and non-zero fractions) through vm_pixel and compares every byte
// with a naive second form (a padded copy of the frame, 64-bit sums); it sends random and extreme view boxes (far outside
// [0, S], infinite, NaN) through vm_box and checks that the frame box lies in the frame.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "view_map.h"

using namespace lp;

static uint32_t rng_state = 2463534242u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rng() & 0xffff) / 65535.0f; }

// the pixel rule on a copy of the frame with a 4-pixel border of 114 all around
static void naive_pixel(const std::vector<uint8_t>& padded, int H, int W, int32_t fx, int32_t fy, uint8_t* out) {
  const int PW = W + 8;
  const long ix = (long)floor((double)fx / 32.0), iy = (long)floor((double)fy / 32.0);
  const long ax = fx - ix * 32, ay = fy - iy * 32;
  for (int ch = 0; ch < 3; ++ch) {
    auto P = [&](long r, long c) -> long long {
      if (r < -4 || r >= H + 4 || c < -4 || c >= W + 4) return 114;
      return padded[((size_t)(r + 4) * PW + (size_t)(c + 4)) * 3 + ch];
    };
    const long long v = P(iy, ix) * (32 - ax) * (32 - ay) + P(iy, ix + 1) * ax * (32 - ay) + P(iy + 1, ix) * (32 - ax) * ay + P(iy + 1, ix + 1) * ax * ay + 512;
    out[ch] = (uint8_t)(v / 1024);
  }
}

static int check_frame(int S, int H, int W) {
  uint8_t* frame = new uint8_t[(size_t)H * W * 3];   // exactly the frame: the sanitizer guards both ends
  for (size_t k = 0; k < (size_t)H * W * 3; ++k) frame[k] = (uint8_t)rng();
  std::vector<uint8_t> padded((size_t)(H + 8) * (W + 8) * 3, 114);
  for (int r = 0; r < H; ++r) memcpy(&padded[((size_t)(r + 4) * (W + 8) + 4) * 3], frame + (size_t)r * W * 3, (size_t)W * 3);
  float* xy = new float[(size_t)S * S * 2];
  int32_t* fixed = new int32_t[(size_t)S * S * 2];
  const float inf = std::numeric_limits<float>::infinity();
  int fails = 0;
  for (int kind = 0; kind < 6; ++kind) {
    for (int j = 0; j < S; ++j)
      for (int i = 0; i < S; ++i) {
        float x, y;
        switch (kind) {
          case 0: x = uniform(-3.f, W + 2.f); y = uniform(-3.f, H + 2.f); break;                          // random
          case 1: x = (float)(W - S + i); y = (float)(H - S + j); break;                                    // ends on the last pixel, fractions 0
          case 2: x = (float)(W - S + i) - 0.5f; y = (float)(H - S + j) - 0.25f; break;                     // ... fractions 16 and 8
          case 3: x = (i & 1) ? 3.0e38f : -3.0e38f; y = (j & 1) ? inf : -inf; break;                        // extreme
          case 4: x = (float)(i % 5 - 2) + (i & 2 ? 0.f : (float)W - 1.f); y = (float)(j % 5 - 2) + (j & 2 ? 0.f : (float)H - 1.f); break;   // the corners
          default: x = (float)W + 1.f - (float)(rng() & 63) / 32.f; y = (float)H + 1.f - (float)(rng() & 63) / 32.f; break;   // the clamp's upper end
        }
        xy[((size_t)j * S + i) * 2] = x; xy[((size_t)j * S + i) * 2 + 1] = y;
      }
    for (size_t k = 0; k < (size_t)S * S; ++k)
      if (!vm_fix(xy[2 * k], W, fixed + 2 * k) || !vm_fix(xy[2 * k + 1], H, fixed + 2 * k + 1)) { printf("FAIL: vm_fix refused a number\n"); ++fails; }
    for (size_t k = 0; k < (size_t)S * S; ++k) {
      if (fixed[2 * k] < -64 || fixed[2 * k] > (W + 1) * 32 || fixed[2 * k + 1] < -64 || fixed[2 * k + 1] > (H + 1) * 32) {
        printf("FAIL: fixed (%d, %d) outside the clamp for a %dx%d frame\n", fixed[2 * k], fixed[2 * k + 1], W, H); ++fails;
      }
      uint8_t got[3], want[3];
      vm_pixel(frame, H, W, fixed[2 * k], fixed[2 * k + 1], got);
      naive_pixel(padded, H, W, fixed[2 * k], fixed[2 * k + 1], want);
      if (memcmp(got, want, 3) != 0 && fails++ < 10)
        printf("FAIL: S %d frame %dx%d kind %d pixel %zu fixed (%d, %d): %d %d %d vs %d %d %d\n", S, W, H, kind, k, fixed[2 * k], fixed[2 * k + 1],
               got[0], got[1], got[2], want[0], want[1], want[2]);
    }
    // boxes through this table: inside the view, far outside, infinite, NaN
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int b = 0; b < 400; ++b) {
      float box[4];
      if (b < 300) { box[0] = uniform(0.f, (float)S); box[2] = uniform(0.f, (float)S); box[1] = uniform(0.f, (float)S); box[3] = uniform(0.f, (float)S); }
      else if (b < 350) { box[0] = uniform(-1e6f, 1e6f); box[1] = uniform(-1e6f, 1e6f); box[2] = uniform(-1e6f, 1e6f); box[3] = uniform(-1e6f, 1e6f); }
      else if (b < 360) { box[0] = -inf; box[1] = -3e38f; box[2] = inf; box[3] = 3e38f; }
      else if (b < 370) { box[0] = nan; box[1] = 1.f; box[2] = 2.f; box[3] = nan; }
      else { box[0] = 0.f; box[1] = 0.f; box[2] = (float)S; box[3] = (float)S; }
      float out[4];
      vm_box(fixed, S, H, W, box, out);
      const bool finite_in = b < 300 || b >= 370;
      if (finite_in && !(out[0] >= 0.f && out[0] <= out[2] && out[2] <= (float)W && out[1] >= 0.f && out[1] <= out[3] && out[3] <= (float)H)) {
        if (fails++ < 10) printf("FAIL: S %d frame %dx%d kind %d box %d -> (%g, %g, %g, %g) leaves the frame\n", S, W, H, kind, b, out[0], out[1], out[2], out[3]);
      }
    }
  }
  int32_t dummy;
  if (vm_fix(std::numeric_limits<float>::quiet_NaN(), W, &dummy)) { printf("FAIL: vm_fix took a NaN\n"); ++fails; }
  delete[] frame;
  delete[] xy;
  delete[] fixed;
  return fails;
}

int main() {
  int fails = 0, frames = 0;
  const int sizes[][3] = {{64, 150, 210}, {64, 70, 720}, {64, 1, 1}, {64, 2, 3}, {2, 5, 4}, {32, 16384, 2}, {32, 3, 16384}, {320, 333, 517}};
  for (const auto& s : sizes) { fails += check_frame(s[0], s[1], s[2]); ++frames; }
  printf("frames %d fails %d\n", frames, fails);
  if (fails) return 1;
  printf("OK\n");
  return 0;
}
