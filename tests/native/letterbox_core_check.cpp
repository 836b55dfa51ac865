// Stand-alone check of csrc/letterbox_core.h (the letterbox resample behind letterbox, window views and evidence pictures),
// built by tests/test_letterbox_core_cpu.py with a plain g++ under -fsanitize=address,undefined.
//
//   letterbox_core_check <dir>      reads <dir>/cases.txt, writes <dir>/<name>.bin per case
//
// A case is one window of one frame and its placement in an OH x OW picture (the Python side computes the placement with the
// references' geometry and compares the dumped pictures with the references' pixels).  For every case the program plays the
// workgroups of the staged form through the header -- span, staging into heap rows of exactly row_cap bytes, resample of four
// pixels per thread -- when the launcher's rule (kind "tile": lb_row_cap / lb_rows_fit per 8 x 128 tile) or the evidence rule
// (kind "evid": the exact span against EV_ROW_CAP, bands of 8 rows) takes that form, and the per-pixel form always.  The frame
// lives at byte offsets 0, 1, 7 and 48 of a heap block that ends with the frame: a read past its last byte or before the
// block is the sanitizer's to report, a read of the lead bytes (a "neighbouring image") is counted by the frame accessor and
// must not happen.  Checked: staged == per-pixel == an independent plain statement of cv2's fixed-point rule, the same
// bytes at every offset, and shift + (b1 - b0) <= row_cap on every staged row.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "letterbox_core.h"

using namespace lp;

static int failures = 0;
#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      if (++failures <= 20) {                    \
        std::printf("FAIL %s: ", #cond);         \
        std::printf(__VA_ARGS__);                \
        std::printf("\n");                       \
      }                                          \
    }                                            \
  } while (0)

struct Case {
  std::string name, kind, frame_file;
  int H, W, x, y, w, h, OH, OW;
  LbPlace g;
};

// the frame's bytes by offset, counting what is asked for outside [0, frame_bytes) before reading it
struct CountingFrame {
  const uint8_t* im;
  long frame_bytes;
  long* outside;
  lb_u32x4 load16(long o) const {
    if (o < 0 || o + 16 > frame_bytes) ++*outside;
    return *reinterpret_cast<const lb_u32x4*>(im + o);
  }
  uint32_t operator[](long o) const {
    if (o < 0 || o >= frame_bytes) ++*outside;
    return im[o];
  }
};
struct CountingRow {   // a window row in the frame
  const CountingFrame* fr;
  long base;
  int operator[](int b) const { return (int)(*fr)[base + b]; }
};

// ---- cv2.resize(INTER_LINEAR) on uint8 and the letterbox around it, stated apart from the header: one coefficient table per
// axis, the window resized as a whole, then pasted into a picture of 114
static void axis_table(int dst, int src, std::vector<int>& idx, std::vector<int>& a0, std::vector<int>& a1) {
  idx.resize(dst); a0.resize(dst); a1.resize(dst);
  const double scale = 1.0 / ((double)dst / (double)src);
  for (int d = 0; d < dst; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    int s = (int)std::floor(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= src - 1) { s = src - 1; f = 0.f; }
    idx[d] = s;
    a1[d] = (int)std::nearbyint(f * 2048.f);   // cvRound: to nearest even
    a0[d] = (int)std::nearbyint((1.f - f) * 2048.f);
  }
}

static std::vector<uint8_t> plain_rule(const std::vector<uint8_t>& frame, const Case& c) {
  std::vector<uint8_t> out((size_t)c.OH * c.OW * 3, 114);
  auto src = [&](int wy, int wx, int ch) { return (int)frame[((size_t)(c.y + wy) * c.W + c.x + wx) * 3 + ch]; };
  const bool copy = c.g.new_w == c.w && c.g.new_h == c.h;
  std::vector<int> xi, xa0, xa1, yi, ya0, ya1;
  axis_table(c.g.new_w, c.w, xi, xa0, xa1);
  axis_table(c.g.new_h, c.h, yi, ya0, ya1);
  for (int dy = 0; dy < c.g.new_h; ++dy)
    for (int dx = 0; dx < c.g.new_w; ++dx)
      for (int ch = 0; ch < 3; ++ch) {
        int v;
        if (copy) {
          v = src(dy, dx, ch);
        } else {
          const int x0 = xi[dx], x1 = std::min(x0 + 1, c.w - 1), y0 = yi[dy], y1 = std::min(y0 + 1, c.h - 1);
          const int top = src(y0, x0, ch) * xa0[dx] + src(y0, x1, ch) * xa1[dx];
          const int bot = src(y1, x0, ch) * xa0[dx] + src(y1, x1, ch) * xa1[dx];
          v = (((ya0[dy] * (top >> 4)) >> 16) + ((ya1[dy] * (bot >> 4)) >> 16) + 2) >> 2;
          v = std::min(std::max(v, 0), 255);
        }
        const int oy = dy + c.g.top, ox = dx + c.g.left;
        if (oy >= 0 && oy < c.OH && ox >= 0 && ox < c.OW) out[((size_t)oy * c.OW + ox) * 3 + ch] = (uint8_t)v;
      }
  return out;
}

// ---- the header's per-pixel form
static std::vector<uint8_t> per_pixel(const CountingFrame& fr, const LbSource& s, const Case& c) {
  std::vector<uint8_t> out((size_t)c.OH * c.OW * 3, 0xEE);
  const bool resize = lb_resizes(s, c.g);
  for (int oy = 0; oy < c.OH; ++oy) {
    const LbRowCoef rc = lb_row_coef(s, c.g, resize, oy);
    const CountingRow r0{&fr, (long)(s.y + rc.sy) * s.pitch + 3L * s.x}, r1{&fr, (long)(s.y + rc.sy1) * s.pitch + 3L * s.x};
    for (int ox = 0; ox < c.OW; ++ox) {
      uint32_t px[3];
      lb_pixel(s, c.g, resize, rc, lin_scale(c.g.new_w, s.w), ox, r0, r1, px);
      for (int ch = 0; ch < 3; ++ch) out[((size_t)oy * c.OW + ox) * 3 + ch] = (uint8_t)px[ch];
    }
  }
  return out;
}

// ---- the header's staged form: workgroups of 256 threads over tiles of LB_TH x tile_w (tile_w = OW: a band)
static std::vector<uint8_t> staged(const CountingFrame& fr, const LbSource& s, const Case& c, int tile_w, int row_cap, int* max_used) {
  std::vector<uint8_t> out((size_t)c.OH * c.OW * 3, 0xEE);
  const bool resize = lb_resizes(s, c.g);
  std::unique_ptr<uint8_t[]> rows[2 * LB_TH];
  for (auto& r : rows) r.reset(new uint8_t[row_cap]);   // exactly row_cap bytes each
  const int groups = tile_w / 4;
  for (int oy0 = 0; oy0 < c.OH; oy0 += LB_TH)
    for (int ox0 = 0; ox0 < c.OW; ox0 += tile_w) {
      int s_shift[2 * LB_TH];
      for (int r = 0; r < 2 * LB_TH; ++r) { s_shift[r] = -1000000; std::memset(rows[r].get(), 0xCD, row_cap); }
      const int dxa = std::max(ox0 - c.g.left, 0), dxb = std::min(std::min(ox0 + tile_w, c.OW) - c.g.left, c.g.new_w);
      LbSpan sp{0, 0};
      if (dxa < dxb) {
        sp = lb_span(s, c.g, resize, dxa, dxb);
        for (int tid = 0; tid < 256; ++tid)
          for (int r = tid >> 4; r < 2 * LB_TH; r += 16) {
            const int shift = lb_stage_row(fr, s, c.g, resize, sp, oy0, r, rows[r].get(), row_cap, tid & 15);
            if (shift < 0) continue;
            s_shift[r] = shift;
            *max_used = std::max(*max_used, shift + sp.b1 - sp.b0);
            EXPECT(shift + (sp.b1 - sp.b0) <= row_cap, "%s tile (%d, %d) row %d: %d bytes in a row of %d", c.name.c_str(), oy0, ox0, r,
                   shift + sp.b1 - sp.b0, row_cap);
          }
      }
      for (int u = 0; u < LB_TH * groups; ++u) {   // a thread = (row j, four adjacent columns)
        const int j = u / groups, ox = ox0 + 4 * (u - j * groups), oy = oy0 + j;
        if (oy >= c.OH || ox >= c.OW) continue;
        const LbRowCoef rc = lb_row_coef(s, c.g, resize, oy);
        const LbRow r0{rows[2 * j].get(), rc.in ? s_shift[2 * j] - sp.b0 : 0}, r1{rows[2 * j + 1].get(), rc.in ? s_shift[2 * j + 1] - sp.b0 : 0};
        uint32_t w3[3];
        lb_resample4(s, c.g, resize, rc, ox, r0, r1, w3);
        for (int b = 0; b < 12; ++b) out[((size_t)oy * c.OW + ox) * 3 + b] = (uint8_t)(w3[b >> 2] >> (8 * (b & 3)));
      }
    }
  return out;
}

static size_t first_diff(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b) {
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i] != b[i]) return i;
  return a.size();
}

static void run_case(const std::string& dir, const Case& c, int* n_staged, int* n_pixel) {
  std::ifstream f(dir + "/" + c.frame_file, std::ios::binary);
  std::vector<uint8_t> frame((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const long frame_bytes = (long)c.H * c.W * 3;
  EXPECT((long)frame.size() == frame_bytes, "%s: frame file of %zu bytes", c.name.c_str(), frame.size());
  if ((long)frame.size() != frame_bytes) return;
  EXPECT(c.OW % 4 == 0 && c.x >= 0 && c.y >= 0 && c.x + c.w <= c.W && c.y + c.h <= c.H, "%s: window", c.name.c_str());
  const std::vector<uint8_t> want = plain_rule(frame, c);

  // which form the device would run
  int tile_w, row_cap;
  if (c.kind == "evid") {   // a band of the E x E picture
    tile_w = c.OW; row_cap = EV_ROW_CAP;
  } else {
    tile_w = LB_TW; row_cap = lb_row_cap(c.w, c.g.new_w, LB_TW);
  }
  for (int off : {0, 1, 7, 48}) {
    std::unique_ptr<uint8_t[]> block(new uint8_t[off + frame_bytes]);   // ends with the frame's last byte
    std::memset(block.get(), 0x5A, off);
    std::memcpy(block.get() + off, frame.data(), frame_bytes);
    long outside = 0;
    const CountingFrame fr{block.get() + off, frame_bytes, &outside};
    const LbSource s{block.get() + off, frame_bytes, 3 * c.W, c.x, c.y, c.w, c.h};
    const bool resize = lb_resizes(s, c.g);
    bool is_staged;
    if (c.kind == "evid") {
      const LbSpan sp = lb_span(s, c.g, resize, 0, c.g.new_w);
      is_staged = sp.b1 - sp.b0 + 32 <= EV_ROW_CAP;
    } else {
      is_staged = lb_rows_fit(row_cap);
    }
    const std::vector<uint8_t> pp = per_pixel(fr, s, c);
    size_t d = first_diff(pp, want);
    EXPECT(d == pp.size(), "%s offset %d: the per-pixel form differs from the plain rule at byte %zu (%d / %d)", c.name.c_str(), off, d, pp[d], want[d]);
    if (is_staged) {
      int used = 0;
      const std::vector<uint8_t> st = staged(fr, s, c, tile_w, row_cap, &used);
      d = first_diff(st, pp);
      EXPECT(d == st.size(), "%s offset %d: the staged form differs from the per-pixel form at byte %zu (%d / %d)", c.name.c_str(), off, d, st[d], pp[d]);
      if (off == 0) std::printf("%s: staged, %d of %d row bytes\n", c.name.c_str(), used, row_cap);
    } else if (off == 0) {
      std::printf("%s: per-pixel only\n", c.name.c_str());
    }
    EXPECT(outside == 0, "%s offset %d: %ld reads outside the frame", c.name.c_str(), off, outside);
    if (off == 0) {
      ++*(is_staged ? n_staged : n_pixel);
      std::ofstream o(dir + "/" + c.name + ".bin", std::ios::binary);
      o.write(reinterpret_cast<const char*>(pp.data()), (std::streamsize)pp.size());
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: letterbox_core_check <dir>\n"); return 2; }
  const std::string dir = argv[1];
  std::ifstream list(dir + "/cases.txt");
  std::string line;
  int n = 0, n_staged = 0, n_pixel = 0;
  while (std::getline(list, line)) {
    std::istringstream in(line);
    Case c;
    if (!(in >> c.name >> c.kind >> c.frame_file >> c.H >> c.W >> c.x >> c.y >> c.w >> c.h >> c.OH >> c.OW >> c.g.new_w >> c.g.new_h >> c.g.top >> c.g.left)) continue;
    run_case(dir, c, &n_staged, &n_pixel);
    ++n;
  }
  // the launchers' rule on its boundary: 16 rows of 4096 bytes fit 64 KiB, 16 rows of 4112 do not
  EXPECT(lb_rows_fit(4096) && !lb_rows_fit(4112), "lb_rows_fit");
  EXPECT(lb_row_cap(1920, 640, LB_TW) == 1200 && lb_row_cap(4480, 416, LB_TW) == 4192, "lb_row_cap");
  std::printf("cases %d staged %d per-pixel %d\n", n, n_staged, n_pixel);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
