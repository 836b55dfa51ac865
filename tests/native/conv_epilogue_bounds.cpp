// Host replay of the residual prefetch of conv3x3_mfma_kernel's epilogue (csrc/conv_kernels.hip, epilogue_tile): which pixel
// of the residual tensor every lane of every wave reads for each of its strip's five patches.  The column choice is the
// kernel's own (csrc/conv_bounds.h); the tensor is a heap array of exactly N x Hout x Wout pixels, so under
// -fsanitize=address,undefined a column outside the row of the last image's last row is a reported overflow as well as a
// failed check.  The expression the kernel used before the clamp is kept as a negative control: it must leave the row at
// Wout = 13 with a 40-column tile (the second wave's strip starts at column 20).
#include <cstdio>
#include <vector>

#include "conv_bounds.h"

// the former base: the strip's first pixel, wherever it lies
static int parent_patch_col(int oxb, int p, int Wout) { return oxb + (oxb + p * 4 < Wout ? p * 4 : 0); }

int main() {
  const int N = 2, Hout = 5;
  long reads = 0, bad_new = 0, bad_parent = 0, bad_parent_13_40 = 0, strips_outside = 0;
  for (int Wout = 1; Wout <= 88; ++Wout) {
    std::vector<int> res((size_t)N * Hout * Wout);   // one int per pixel: its own column
    for (int n = 0; n < N; ++n)
      for (int y = 0; y < Hout; ++y)
        for (int x = 0; x < Wout; ++x) res[((size_t)n * Hout + y) * Wout + x] = x;
    for (int TW = 20; TW <= 40; TW += 20) {
      const int bww = TW / 20, bwh = 2, TH = 4 * bwh;
      const int tiles_x = (Wout + TW - 1) / TW, tiles_y = (Hout + TH - 1) / TH;
      for (int n = 0; n < N; ++n)
        for (int ty = 0; ty < tiles_y; ++ty)
          for (int tx = 0; tx < tiles_x; ++tx)
            for (int wave = 0; wave < bwh * bww; ++wave)
              for (int lane = 0; lane < 64; ++lane) {
                // conv3x3_mfma_kernel's lane -> pixel map
                const int col = lane & 15;
                const int wy = bww == 2 ? wave >> 1 : wave, wx = wave - wy * bww;
                const int oy = ty * TH + wy * 4 + (col >> 2);
                const int oxb = tx * TW + wx * 20 + (col & 3);
                if (oy >= Hout) continue;   // epilogue_tile returns before any load
                strips_outside += oxb >= Wout;
                for (int p = 0; p < 5; ++p) {
                  const int c = lp::residual_patch_col(oxb, p, Wout);
                  ++reads;
                  if (c < 0 || c >= Wout) { ++bad_new; continue; }
                  const int got = res[((size_t)n * Hout + oy) * Wout + c];   // the load itself, in bounds of the heap array
                  if (got != c) ++bad_new;
                  // a patch inside the image must read its own pixel
                  if (oxb + p * 4 < Wout && c != oxb + p * 4) ++bad_new;
                  const int cp = parent_patch_col(oxb, p, Wout);
                  if (cp >= Wout) {
                    ++bad_parent;
                    if (Wout == 13 && TW == 40) ++bad_parent_13_40;
                  } else if (cp != c) {
                    ++bad_new;   // where the former expression was inside the row the clamp changes nothing
                  }
                }
              }
    }
  }
  printf("reads %ld, strips right of the image %ld, out of range: clamped %ld, former %ld (Wout 13, TW 40: %ld)\n", reads,
         strips_outside, bad_new, bad_parent, bad_parent_13_40);
  if (bad_new != 0) { printf("FAIL: the clamped column leaves the row\n"); return 1; }
  if (bad_parent_13_40 == 0) { printf("FAIL: the negative control found nothing at Wout 13, TW 40\n"); return 1; }
  printf("ok\n");
  return 0;
}
