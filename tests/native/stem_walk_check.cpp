// csrc/stem_walk.h without a device (tests/test_stem_walk_cpu.py builds this with g++ -fsanitize=address,undefined and runs it).
//   walks   for both geometries and every wave, lane (column and K group) and iteration: the incremental read / write offsets
//           equal the closed forms, every LDS read (with the two further dwords of the gather) lies inside in_tile, every write
//           inside st_tile, and the peeled iterations are exactly those in which some lane is not live
//   stage   for the given image sizes and every tile: the staged tile equals "row r = image row 4 oy0 - 3 + r, dword c = row dword
//           w0 + c, zero outside", every tile dword is written (twice only in the tile's last row, by writers that agree) and every loaded image
//           dword lies inside the image
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "stem_walk.h"

using namespace lp::swalk;

static long n_checks = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    ++n_checks;                                         \
    if (!(c)) {                                         \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
      std::printf(__VA_ARGS__);                         \
      std::printf("\n");                                \
      std::exit(1);                                     \
    }                                                   \
  } while (0)

// the iterations in which every lane of every wave is live must be the first W::FULL, the rest are peeled
template <class W, class Pos>
static void check_peel(Pos pos_of, int walkers) {
  for (int i = 0; i < W::ITERS; ++i) {
    bool all_live = true;
    for (int wave = 0; wave < kWaves; ++wave)
      for (int col = 0; col < 16; ++col)
        for (int s = 0; s < walkers; ++s) all_live = all_live && pos_of(wave, col, s) + W::STEP * i < W::N;
    CHECK(all_live == (i < W::FULL), "iteration %d: all live %d, FULL %d", i, (int)all_live, W::FULL);
  }
  // every position of the tile is taken exactly once
  std::vector<int> seen(W::N, 0);
  for (int i = 0; i < W::ITERS; ++i)
    for (int wave = 0; wave < kWaves; ++wave)
      for (int col = 0; col < 16; ++col)
        for (int s = 0; s < walkers; ++s) {
          const int pos = pos_of(wave, col, s) + W::STEP * i;
          if (pos < W::N) ++seen[pos];
        }
  for (int p = 0; p < W::N; ++p) CHECK(seen[p] == 1, "position %d taken %d times", p, seen[p]);
}

static void check_pair_walk() {
  typedef PairWalk W;
  typedef W::G G;
  check_peel<W>([](int wave, int col, int) { return W::pos0(wave, col); }, 1);
  for (int wave = 0; wave < kWaves; ++wave)
    for (int lane = 0; lane < kLane; ++lane) {
      const int g = lane >> 4, col = lane & 15, ky0 = 2 * (g & 1), h = g >> 1;
      const int pos0 = W::pos0(wave, col);
      Walk w = start<W>(pos0, W::lane_rd(g), W::lane_wr(g));
      for (int i = 0; i < W::ITERS; ++i, advance<W>(w)) {
        const int pos = pos0 + W::STEP * i;
        const bool live = pos < W::N;
        CHECK(live || i >= W::FULL, "dead lane in an unpeeled iteration %d", i);
        const Walk q = live ? w : last<W>(W::lane_rd(g), W::lane_wr(g));
        const int r = live ? pos / W::PER_ROW : W::ROWS - 1, p = live ? pos % W::PER_ROW : W::PER_ROW - 1;
        CHECK(q.r == r && q.p == p, "wave %d lane %d it %d: (%d, %d) != (%d, %d)", wave, lane, i, q.r, q.p, r, p);
        // K step 0: row 2 r + ky0, step 1: row 2 r + 1; dword 3 p + 2 h of it and the two behind
        for (int s = 0; s < 2; ++s) {
          const int off = s == 0 ? q.rd : q.rd + W::rd1(g), ky = s == 0 ? ky0 : 1;
          CHECK(off % 4 == 0 && off / 4 == (2 * r + ky) * G::ROWW + 3 * p + 2 * h, "wave %d lane %d it %d step %d: read offset %d", wave, lane, i, s, off);
          CHECK(off >= 0 && off / 4 + 2 < G::IN_DWORDS, "read %d outside in_tile", off);
          CHECK((off / 4 + 2) / G::ROWW == 2 * r + ky, "read %d leaves its row", off);
        }
        const int c = 2 * p + h;
        if (live && c < G::SW) {
          CHECK(q.wr == (r * G::LW + c) * 16 + (g & 1) * 8, "wave %d lane %d it %d: write offset %d", wave, lane, i, q.wr);
          CHECK(q.wr >= 0 && q.wr + 8 <= G::ST_BYTES, "write %d outside st_tile", q.wr);
        }
      }
    }
}

template <int TH>
static void check_pixel_walk() {
  typedef PixelWalk<TH> W;
  typedef typename W::G G;
  check_peel<W>([](int wave, int col, int s) { return W::pos0(wave, col, s); }, 2);
  for (int wave = 0; wave < kWaves; ++wave)
    for (int lane = 0; lane < kLane; ++lane)
      for (int second = 0; second < 2; ++second) {
        const int g = lane >> 4, col = lane & 15;
        const int pos0 = W::pos0(wave, col, second);
        Walk w = start<W>(pos0, W::lane_rd(g), W::lane_wr(g));
        for (int i = 0; i < W::ITERS; ++i, advance<W>(w)) {
          const int pos = pos0 + W::STEP * i;
          const bool live = pos < W::N;
          CHECK(live || i >= W::FULL, "dead lane in an unpeeled iteration %d", i);
          const Walk q = live ? w : last<W>(W::lane_rd(g), W::lane_wr(g));
          const int r = live ? pos / W::PER_ROW : W::ROWS - 1, p = live ? pos % W::PER_ROW : W::PER_ROW - 1;
          CHECK(q.r == r && q.p == p, "wave %d lane %d it %d: (%d, %d) != (%d, %d)", wave, lane, i, q.r, q.p, r, p);
          // K group g < 3: three consecutive dwords of window row g from byte 3 + 6 p; g == 3: the dword two further on of the three rows
          const int bo = 3 + 6 * p;
          CHECK((q.rd & 3) == (bo & 3), "byte shift %d != %d", q.rd & 3, bo & 3);
          for (int k = 0; k < 3; ++k) {
            const int off = (q.rd & ~3) + k * W::kstride4(g);
            const int row = 2 * r + (g < 3 ? g : k), dw = (bo >> 2) + (g < 3 ? k : 2);
            CHECK(off / 4 == row * G::ROWW + dw, "wave %d lane %d it %d k %d: read offset %d", wave, lane, i, k, off);
            CHECK(off >= 0 && off / 4 < G::IN_DWORDS && dw < G::ROWW && row < G::IR, "read %d outside in_tile", off);
          }
          if (live) {
            CHECK(q.wr == (g >> 1) * G::ST_BYTES + (r * G::LW + p) * 16 + (g & 1) * 8, "wave %d lane %d it %d: write offset %d", wave, lane, i, q.wr);
            CHECK(q.wr >= 0 && q.wr + 8 <= 2 * G::ST_BYTES, "write %d outside st_tile", q.wr);
          }
        }
      }
}

template <class G>
static void check_stage(int Hin, int Win) {
  CHECK(Win % 4 == 0, "width %d", Win);
  const int row_words = Win * 3 / 4;
  const int H1 = (Hin + 1) / 2, W1 = (Win + 1) / 2, H2 = (H1 + 1) / 2, W2 = (W1 + 1) / 2;
  long tiles = 0;
  for (int by = 0; by < (H2 + G::TH - 1) / G::TH; ++by)
    for (int bx = 0; bx < (W2 + G::TW - 1) / G::TW; ++bx, ++tiles) {
      const int oy0 = by * G::TH, ox0 = bx * G::TW;
      std::vector<long> tile(G::IN_DWORDS, -2);   // -2: never written, -1: zero, else the image dword
      for (int wave = 0; wave < kWaves; ++wave)
        for (int lane = 0; lane < kLane; ++lane)
          for (int k = 0; k < stage_rows<G>(); ++k) {
            const StageSrc s = stage_src<G>(wave, lane, k, oy0, ox0, Hin, row_words);
            CHECK(s.gidx >= 0 && s.gidx < (long)Hin * row_words, "tile (%d, %d): load of dword %ld outside the image", oy0, ox0, s.gidx);
            if (!s.store) continue;
            const int r = stage_row<G>(wave, k);
            CHECK(r >= 0 && r < G::IR, "tile (%d, %d): row %d outside the tile", oy0, ox0, r);
            long& d = tile[r * G::ROWW + stage_col(wave, lane)];
            const long v = s.keep ? s.gidx : -1;
            // (the tile's last row is staged by two waves: they must agree)
            CHECK(d == -2 || (d == v && r == G::IR - 1), "tile (%d, %d): dword written twice, %ld and %ld", oy0, ox0, d, v);
            d = v;
          }
      for (int r = 0; r < G::IR; ++r)
        for (int c = 0; c < G::ROWW; ++c) {
          const int iy = 4 * oy0 - 3 + r, wi = ((12 * ox0 - 9) >> 2) + c;
          const long want = (iy >= 0 && iy < Hin && wi >= 0 && wi < row_words) ? (long)iy * row_words + wi : -1;
          CHECK(tile[r * G::ROWW + c] == want, "%d x %d tile (%d, %d) row %d dword %d: %ld, want %ld", Hin, Win, oy0, ox0, r, c, tile[r * G::ROWW + c], want);
        }
    }
  std::printf("stage %dx%d tiles %ld\n", Hin, Win, tiles);
}

int main() {
  check_pair_walk();
  std::printf("pair_walk iters %d full %d\n", PairWalk::ITERS, PairWalk::FULL);
  check_pixel_walk<8>();
  std::printf("pixel_walk iters %d full %d\n", PixelWalk<8>::ITERS, PixelWalk<8>::FULL);
  const int sizes[][2] = {{640, 640}, {352, 352}, {384, 640}, {64, 64}};
  for (const auto& s : sizes) check_stage<Geo<8>>(s[0], s[1]);
  std::printf("ok %ld checks\n", n_checks);
  return 0;
}
