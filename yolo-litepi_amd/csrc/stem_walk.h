// Geometry of the two fused network-head kernels (conv_kernels.hip: stem_block_kernel, stem_block16_kernel): how the uint8 tile is
// staged by rows, and how a lane walks the stem's pixel pairs (v1) or pixels (v2) with one LDS read offset and one st_tile write
// offset that advance by a constant per iteration, with one correction at the row wrap.  Pure: no HIP, no environment, constexpr
// functions only -- the kernels call them on the device, and tests/native/stem_walk_check.cpp checks them with a plain C++
// compiler: the steps against the closed forms they come from, every LDS index against the arrays, the staging map against its
// definition.
#pragma once

namespace lp {
namespace swalk {

constexpr int kWaves = 4, kLane = 64;

// ---- the tile: TH x 32 outputs of the stride-2 conv <- SH x SW stem pixels <- IR input rows of ROWW dwords ------------------
template <int TH_>
struct Geo {
  static constexpr int TH = TH_, TW = 32;
  static constexpr int SH = 2 * TH + 1, SW = 2 * TW + 1;   // stem rows, columns
  static constexpr int LW = 65;                            // st_tile row pitch, pixels of 16 B
  static constexpr int IR = 2 * SH + 1;                    // input rows
  static constexpr int ROWW = 102;                         // dwords per staged input row: 3 + 131 * 3 bytes + a lane's third dword
  static constexpr int IN_DWORDS = IR * ROWW;
  static constexpr int ST_BYTES = SH * LW * 16;            // one plane of 8 fp16 channels
};

constexpr int clampi(int x, int n) { return x < 0 ? 0 : (x < n ? x : n - 1); }
constexpr bool inside(int x, int n) { return x >= 0 && x < n; }

// ---- staging: tile row r = image row 4 oy0 - 3 + r, tile dword c = row dword w0 + c, zero outside the image --------------------
// A wave owns half rows: wave w stages dwords [64 (w & 1), 64 (w & 1) + 64) of the rows (w >> 1) + 2 k, k = 0 .. stage_rows() - 1.
// Row number, clamp, validity and base address depend on (w, k) alone -- wave-uniform, scalar registers; a lane's dword column,
// its clamp and its validity do not depend on k.  IR is odd: the last row of the odd-row waves would lie below the tile; they
// stage the tile's last row once more instead (the same dwords from the same addresses as the even-row waves write there), so
// that no load and no store of the staging is conditional -- a conditional last store took its load behind the other stores.
constexpr int tile_iy0(int oy0) { return 4 * oy0 - 3; }
constexpr int tile_w0(int ox0) { return (12 * ox0 - 9) >> 2; }    // first byte (4 ox0 - 3) * 3 = 3 mod 4: tile byte 3 is that byte
template <class G> constexpr int stage_rows() { return (G::IR + 1) / 2; }
template <class G> constexpr int stage_row(int wave, int k) {
  const int r = (wave >> 1) + 2 * k;
  return 2 * k + 1 < G::IR ? r : (r < G::IR ? r : G::IR - 1);   // (the clamp can only bind for the last k: a constant test for the others)
}
constexpr int stage_col(int wave, int lane) { return (wave & 1) * kLane + lane; }

// what lands in tile dword (stage_row, stage_col) -- the kernels do exactly this, with the row part on the scalar unit
struct StageSrc {
  bool store;   // the dword exists in the tile (column < ROWW)
  bool keep;    // it lies inside the image; otherwise zero is stored
  long gidx;    // the image dword that is LOADED (always inside the image: clamped row, clamped column)
};
template <class G>
constexpr StageSrc stage_src(int wave, int lane, int k, int oy0, int ox0, int Hin, int row_words) {
  const int r = stage_row<G>(wave, k), c = stage_col(wave, lane);
  const int iy = tile_iy0(oy0) + r, wi = tile_w0(ox0) + c;
  return StageSrc{c < G::ROWW, inside(iy, Hin) && inside(wi, row_words), (long)clampi(iy, Hin) * row_words + clampi(wi, row_words)};
}

// ---- the walks ----------------------------------------------------------------------------------------------------------------
// A wave takes one MFMA tile of 16 positions per step; positions are numbered row-major over the stem tile (PER_ROW per row).
// STEP positions further on = one row down and STEP - PER_ROW along (STEP - PER_ROW < PER_ROW), and once more a row down where
// that leaves the row: Walk::advance.
struct Walk {
  int r, p;      // stem row, position in the row
  int rd, wr;    // LDS read offset, st_tile write offset (units: see the geometry)
};
template <class W>
constexpr void advance(Walk& w) {
  w.p += W::STEP - W::PER_ROW;
  w.r += 1;
  w.rd += W::RD_STEP;
  w.wr += W::WR_STEP;
  if (w.p >= W::PER_ROW) {
    w.p -= W::PER_ROW;
    w.r += 1;
    w.rd += W::RD_WRAP;
    w.wr += W::WR_WRAP;
  }
}
template <class W>
constexpr Walk start(int pos, int lane_rd, int lane_wr) {
  const int r = pos / W::PER_ROW, p = pos - r * W::PER_ROW;   // (once per lane, before the loop)
  return Walk{r, p, W::rd_of(r, p) + lane_rd, W::wr_of(r, p) + lane_wr};
}
// the walker of a lane that is not live in a peeled iteration reads where the last position of the tile reads and stores nothing
template <class W>
constexpr Walk last(int lane_rd, int lane_wr) {
  return Walk{W::ROWS - 1, W::PER_ROW - 1, W::rd_of(W::ROWS - 1, W::PER_ROW - 1) + lane_rd, W::wr_of(W::ROWS - 1, W::PER_ROW - 1) + lane_wr};
}

// v1, stem_block_kernel: positions are pixel PAIRS (two pixels per MFMA column), 33 per stem row; a wave's tiles are 4 apart.
//   rd: BYTE offset into in_tile of the dword that holds window byte 3 + 12 p of input row 2 r (the lane adds 4 (ky * ROWW + 2 h)
//       for its first K step; its second step reads row 1, a per-lane constant further on)
//   wr: byte offset into st_tile of pixel (r, 2 p) (the lane adds 16 (g >> 1) + 8 (g & 1))
constexpr int pair_rd(int r, int p) { return 4 * (2 * r * Geo<8>::ROWW + 3 * p); }
constexpr int pair_wr(int r, int p) { return (r * Geo<8>::LW + 2 * p) * 16; }
struct PairWalk {
  typedef Geo<8> G;
  static constexpr int ROWS = G::SH, PER_ROW = (G::SW + 1) / 2, N = ROWS * PER_ROW, NTILE = (N + 15) / 16;
  static constexpr int STEP = 16 * kWaves;
  static constexpr int ITERS = (NTILE + kWaves - 1) / kWaves;   // per wave
  static constexpr int FULL = (N / 16) / kWaves;                // leading iterations in which every lane of every wave is live
  static constexpr int rd_of(int r, int p) { return pair_rd(r, p); }
  static constexpr int wr_of(int r, int p) { return pair_wr(r, p); }
  static constexpr int RD_STEP = pair_rd(1, STEP - PER_ROW), WR_STEP = pair_wr(1, STEP - PER_ROW);
  static constexpr int RD_WRAP = pair_rd(1, -PER_ROW), WR_WRAP = pair_wr(1, -PER_ROW);
  static constexpr int pos0(int wave, int col) { return wave * 16 + col; }
  // lane group g = K group: step 0 reads window row ky0 = 2 (g & 1), byte half h = g >> 1; step 1 reads row 1, rd1 further on.
  // The lane's stem pixel is the pair's pixel h; it holds channels 4 (g & 1) .. + 3 of it
  static constexpr int lane_rd(int g) { return 4 * (2 * (g & 1) * G::ROWW + 2 * (g >> 1)); }
  static constexpr int rd1(int g) { return 4 * (1 - 2 * (g & 1)) * G::ROWW; }
  static constexpr int lane_wr(int g) { return (g >> 1) * 16 + (g & 1) * 8; }
};
static_assert(PairWalk::STEP - PairWalk::PER_ROW >= 0 && PairWalk::STEP - PairWalk::PER_ROW < PairWalk::PER_ROW, "one wrap per step at most");
static_assert(PairWalk::RD_STEP == 4 * 297 && PairWalk::RD_WRAP == 4 * 105 && PairWalk::WR_STEP == 2032 && PairWalk::WR_WRAP == -16, "pair walk steps");
static_assert(PairWalk::ITERS == 9 && PairWalk::FULL == 8, "pair walk: one peeled iteration");

// v2, stem_block16_kernel<TH>: positions are PIXELS, 65 per stem row; a wave takes tiles t and t + 4 per iteration (two walkers,
// 64 positions apart), iterations are 8 tiles apart.
//   rd: BYTE offset into in_tile of the first window byte 3 + 6 p of input row 2 r (dword = rd >> 2, byte shift = rd & 3)
//   wr: byte offset into a plane of st_tile of pixel (r, p) -- LW == SW: 16 x the position
template <class G> constexpr int pixel_rd(int r, int p) { return 8 * r * G::ROWW + 3 + 6 * p; }
template <class G> constexpr int pixel_wr(int r, int p) { return (r * G::LW + p) * 16; }
template <int TH_>
struct PixelWalk {
  typedef Geo<TH_> G;
  static constexpr int ROWS = G::SH, PER_ROW = G::SW, N = ROWS * PER_ROW, NTILE = (N + 15) / 16;
  static constexpr int STEP = 32 * kWaves;
  static constexpr int ITERS = (NTILE + 2 * kWaves - 1) / (2 * kWaves);   // per wave
  static constexpr int FULL = (N / 16) / (2 * kWaves);                    // leading iterations with both tiles of every wave all live
  static constexpr int rd_of(int r, int p) { return pixel_rd<G>(r, p); }
  static constexpr int wr_of(int r, int p) { return pixel_wr<G>(r, p); }
  static constexpr int RD_STEP = pixel_rd<G>(1, STEP - PER_ROW) - pixel_rd<G>(0, 0), WR_STEP = pixel_wr<G>(1, STEP - PER_ROW);
  static constexpr int RD_WRAP = pixel_rd<G>(1, -PER_ROW) - pixel_rd<G>(0, 0), WR_WRAP = pixel_wr<G>(1, -PER_ROW);
  static constexpr int pos0(int wave, int col, int second) { return (wave + 4 * second) * 16 + col; }
  // K group g < 3: bytes 0..7 of window row g (three consecutive dwords); g == 3: byte 8 of the three rows (the dword two further
  // on in each row) -- one address form: the lane's base + k * kstride4.  Channels 4g .. 4g+3: plane g >> 1, bytes 8 (g & 1)
  static constexpr int lane_rd(int g) { return 4 * (g < 3 ? g * G::ROWW : 2); }
  static constexpr int kstride4(int g) { return 4 * (g < 3 ? 1 : G::ROWW); }
  static constexpr int lane_wr(int g) { return (g >> 1) * G::ST_BYTES + (g & 1) * 8; }
};
static_assert(PixelWalk<8>::STEP - PixelWalk<8>::PER_ROW >= 0 && PixelWalk<8>::STEP - PixelWalk<8>::PER_ROW < PixelWalk<8>::PER_ROW, "one wrap per step at most");
static_assert(PixelWalk<8>::RD_STEP == 1194 && PixelWalk<8>::RD_WRAP == 426 && PixelWalk<8>::WR_STEP == 2048 && PixelWalk<8>::WR_WRAP == 0, "pixel walk steps");
static_assert(PixelWalk<8>::ITERS == 9 && PixelWalk<8>::FULL == 8, "pixel walk: one peeled iteration");

}  // namespace swalk
}  // namespace lp
