// Planner and weight-stream packer of the fused Detect head (head_kernels.hip), and the table of its instantiated variants.
// Host-only and pure: no HIP, no allocation on a device, no environment -- a plain C++ compiler builds it, and
// tests/native/head_plan_replay.cpp replays it against a recording (tests/golden/head_plans.json).
// HeadLayer (head.h) derives from HeadPlan: its build() is "plan, pack, upload", its launch() an index into the table below, which
// is also what gets instantiated.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "f16.h"

namespace lp {
namespace hplan {

// The kernel-shape switches of a load (PlanSwitches, detector_plan.cpp, reads them from the environment)
struct HeadSwitches {
  bool merged_a = false;   // LITEPI_HEAD_MERGED_A: the merged stage A on every shape (A/B lever of the split stage A)
  bool a32 = false;        // LITEPI_HEAD_A32: round 3's stage A (32-pixel slots)
  bool two_wg = false;     // LITEPI_HEAD_2WG: the two-workgroup shapes of round 2
  bool one_wg = false;     // LITEPI_HEAD_1WG: the one-workgroup shapes
  int flags = 0;           // LITEPI_HEAD_FLAGS: HeadArgs::flags (1 = s_setprio 1 in the K loops, 2 = in the epilogues)
};

// split stage A: a pass of rtp row tiles per half-step puts as many K steps (2 rtp fragments each) into a chunk as a slot addresses
// -- fragment 7 of an 8-fragment slot is not addressable -- and as divide the 9 spt steps of the conv
constexpr int steps_per_chunk(int slotf, int rtp, int spt) {
  int d = (slotf == 8 ? 7 : slotf) / (2 * rtp);
  while (d > 1 && (9 * spt) % d != 0) --d;
  return d;
}

// (the workgroup's vote word needs no bytes of its own: it is the padding slot of MID pixel 0)
constexpr size_t head_lds(int th, int tw, int kpt, int c3t, int slotf, bool ovl) {
  const size_t in_b = (size_t)(th + 4) * (tw + 4) * (2 * kpt + 1) * 16, mid_b = (size_t)(th + 2) * (tw + 2) * (4 * (2 + c3t) + 1) * 16;
  const size_t in = (in_b + 1023) & ~(size_t)1023, mid = (mid_b + 1023) & ~(size_t)1023;
  // slotf 8: MID overlays the input tile; slots 64 B short of 8 KiB (kchunk): 53,696 B = 42 LDS granules of 1280 B
  if (slotf == 8) return (in_b > mid_b ? in_b : mid_b) + 2 * (size_t)(8192 - 64);
  if (ovl) return (in > mid ? in : mid) + 2 * (size_t)slotf * 1024;
  return in + mid + 2 * (size_t)slotf * 1024;
}

// One row per head_fused_kernel instantiation: class row tiles c3t and K steps per tap kpt = Cin / 16 select it; tile shape th x tw,
// pixel tiles per wave in stage A / B (ceil((th+2)(tw+2)/32) <= 4*pa, ceil(th*tw/32) <= 4*pb), K steps per stage-A chunk ksa (a
// divisor of 9*kpt with (2+c3t)*ksa <= slotf fragments), fragments per weight-ring slot slotf, input-tile rows per wave nrw.
// Chosen for LDS (input tile + first-conv image + 48 KiB ring <= 160 KiB) and for whole tiles on the 80 / 40 / 20 maps of a 640 input;
// other map sizes run the same shapes with masked edges.  The v1 P3 entries with an 8 x 16 tile and one pixel tile per wave in
// stage B share a CU: the VALU phases (SiLU epilogues, decode: transcendental-bound) and the prologue of one workgroup run under the
// MFMA phases of the others -- with one workgroup per CU the matrix pipe idles through them.  slotf 12: two per CU (80 KiB, <= 256
// registers; round 2).  slotf 8: THREE per CU (round 3: 98 us per launch against 112): MID overlays the input tile, 8-fragment
// slots 64 bytes short of 8 KiB (the LDS granule is 1280 B: 42 granules = 53,760 B per workgroup is the limit, measured with
// tools/ubench/lds_occupancy.hip; MID + two whole slots would be 53,824), the projections as two chunks, and 168 registers --
// reached by requesting what only the decode needs (anchors, geometry, DFL weights) late: behind stage A at first, now behind the vote.
// ov: MID overlays the input tile in LDS.
// a16 (round 4): stage A on 16x16x32 MFMAs -- pa counts 16-pixel tiles per wave, ksa half-steps per chunk (one tap per chunk).
// split (a16 only): the class tower's first conv alone in front of the vote, the box tower's behind it in the workgroups that stay;
// the chunk sizes of the two passes follow from the slot size (steps_per_chunk).
// The kernel's other template arguments are functions of these where that reproduces every instantiation; nrw is not (ceil((th+4)/4)
// would give 4 on the 10 x 10 tiles, and only some of them are instantiated with 4).
struct HeadVariant {
  int c3t, kpt, th, tw, pa, pb, ksa, slotf, nrw;
  bool ov, a16, split;
  constexpr int rt() const { return 2 + c3t; }          // row tiles (32 channels) of the merged first convs: box 2 | class c3t
  constexpr int spt() const { return (kpt + 1) / 2; }   // a16: K steps of 32 channels per tap (Cin = 16 mod 32: the last one half zero weights)
  constexpr int npc() const { return ((tw + 4) * (2 * kpt + 1) + 63) / 64; }   // 64-slot pieces per input-tile row
  constexpr int nca() const { return a16 && !split ? 9 * spt() / (ksa / 2) : 9; }   // stage-A chunks of the merged a16 path (else unused: 9)
  constexpr int kc() const { return steps_per_chunk(slotf, c3t, spt()); }   // split: K steps per chunk of the class | box pass
  constexpr int kb() const { return steps_per_chunk(slotf, 2, spt()); }
  constexpr int ksac() const { return split ? 2 * kc() : 0; }   // split: half-steps per chunk and chunks of the class | box pass
  constexpr int ncac() const { return split ? 9 * spt() / kc() : 0; }
  constexpr int ksab() const { return split ? 2 * kb() : 0; }
  constexpr int ncab() const { return split ? 9 * spt() / kb() : 0; }
  constexpr size_t lds_bytes() const { return head_lds(th, tw, kpt, c3t, slotf, ov); }
  // what the kernel's chunk counter walks through: stage A, the class tower, its projection, the box tower, its projection
  constexpr int nchunks() const {
    const int nc_a = split ? ncac() + ncab() : (a16 ? 9 * spt() / (ksa / 2) : 9 * kpt / ksa);
    const int nc_c = c3t == 2 ? 36 / (slotf / 2) : 18 / (slotf >= 18 ? 18 : 6);
    return nc_a + nc_c + 1 + 36 / (slotf / 2) + 1;
  }
  // selectable under a load's switches; plan_head takes the FIRST selectable row of (c3t, kpt), so the order below is behaviour
  constexpr bool selectable(const HeadSwitches& sw) const {
    return !(sw.one_wg && slotf <= 12) && !(ov && sw.two_wg) && !(a16 && (sw.a32 || sw.one_wg || sw.two_wg)) && !(split && sw.merged_a);
  }
  // nullptr, or what is inconsistent about the row
  constexpr const char* check() const {
    const int lim = slotf == 8 ? 7 : slotf;   // fragment 7 of an 8-fragment slot is not addressable
    if (slotf != 8 && slotf != 12 && slotf != 24) return "slots of 8, 12 or 24 fragments only";
    if (slotf == 8 && c3t != 1) return "fragment 7 of an 8-fragment slot: only the box tower's chunks and the box projection";
    // chunks hold at most slotf fragments (one ring slot): stage A ksa K steps x rt row tiles, stage B box 12 x 2, class 18 x 1
    // (12 x 2 for two class row tiles), projections 2 (4) and 8
    if (ksa % 2 == 0 && 9 * kpt / ksa < 2) return "stage A needs two chunks";
    if (split && !a16) return "the split stage A exists on 16-pixel tiles only";
    if (split && (kc() < 1 || kb() < 1)) return "a K step of the split stage A does not fit a ring slot";
    if (a16) {   // a chunk is ksa half-steps = ksa / 2 K steps x two row halves
      if (ksa % 2 != 0 || (9 * spt()) % (ksa / 2) != 0 || rt() * ksa > lim || (th + 2) * (tw + 2) > 64 * pa) return "inconsistent 16-pixel-tile configuration";
      // odd kpt: the zeroed guard slot behind the tile lies inside MID's span
      if (kpt % 2 != 0 && !(ov && (size_t)(th + 4) * (tw + 4) * (2 * kpt + 1) + 1 <= (size_t)(th + 2) * (tw + 2) * (4 * rt() + 1)))
        return "odd K steps per tap on 16-pixel tiles need the guard slot inside MID";
    } else {
      if ((9 * kpt) % ksa != 0 || rt() * ksa > slotf || (th + 2) * (tw + 2) > 128 * pa) return "inconsistent stage A";
    }
    if (lds_bytes() > (slotf == 8 ? 53760u : (slotf == 12 ? 80u * 1024 : 160u * 1024))) return "LDS over the shape's workgroups-per-CU limit";
    if (th + 4 > (slotf <= 12 && !(ov && slotf == 12) ? 12 : (ov ? 16 : 20)) || th + 4 > 4 * nrw) return "input tile too tall";
    if (th * tw > 128 * pb) return "stage B: more pixel tiles than the waves hold";
    if (nchunks() > 64 || nchunks() * slotf >= 65536) return "weight stream too long";
    return nullptr;
  }
};

constexpr HeadVariant kHeadVariants[] = {
    // c3t kpt th  tw pa pb ksa slotf nrw ov    a16   split
    {1, 2, 8, 16, 3, 1, 2, 8, 3, true, true, true},       // v1 P3: Cin 32, THREE workgroups per CU, stage A on 16-pixel tiles (12 for 180 pixels)
    {1, 2, 8, 16, 3, 1, 2, 8, 3, true, true, false},      //   ... with the merged stage A (LITEPI_HEAD_MERGED_A)
    {1, 4, 10, 20, 5, 2, 4, 12, 4, true, true, true},     // v1 P4: Cin 64, TWO workgroups per CU, 17 tiles of 16 for 264 pixels
    {1, 4, 10, 20, 5, 2, 4, 12, 4, true, true, false},
    {1, 8, 10, 10, 3, 1, 8, 24, 5, false, true, true},    // v1 P5: Cin 128, 9 tiles of 16 for 144 pixels
    {1, 8, 10, 10, 3, 1, 8, 24, 5, false, true, false},
    {2, 3, 8, 16, 3, 1, 2, 12, 3, true, true, true},      // v2 P3: Cin 48 (K padded to 64 per tap), 48-channel class tower, TWO workgroups per CU (73.5 KB)
    {2, 3, 8, 16, 3, 1, 2, 12, 3, true, true, false},
    {2, 6, 10, 10, 3, 1, 2, 12, 4, true, true, true},     // v2 P4: Cin 96, 9 tiles of 16 for 144 pixels; MID over the input tile + 12-fragment slots: 64.8 KB, TWO per CU
    {2, 6, 10, 10, 3, 1, 2, 12, 4, true, true, false},
    {2, 12, 10, 10, 3, 1, 6, 24, 4, true, true, false},   // v2 P5: Cin 192, 10 x 10 tiles (256 workgroups = one round; MID over the input tile: 126 KB); merged stage A: split measured slower
    {1, 2, 8, 16, 2, 1, 2, 8, 3, true, false, false},     // v1 P3, round 3's shape: stage A on 32-pixel slots (LITEPI_HEAD_A32)
    {1, 2, 8, 16, 2, 1, 2, 12, 3, false, false, false},   // v1 P3: Cin 32, two workgroups per CU (LITEPI_HEAD_2WG)
    {1, 2, 16, 16, 3, 2, 6, 24, 5, false, false, false},  // v1 P3: Cin 32 (LITEPI_HEAD_1WG)
    {1, 4, 10, 20, 3, 2, 4, 12, 4, true, false, false},   // v1 P4: Cin 64, TWO workgroups per CU (MID over the input tile: 79.5 KB; LITEPI_HEAD_A32)
    {1, 4, 10, 20, 3, 2, 6, 24, 5, false, false, false},  // v1 P4: Cin 64 (LITEPI_HEAD_2WG / LITEPI_HEAD_1WG)
    {1, 8, 10, 10, 2, 1, 8, 24, 5, false, false, false},  // v1 P5: Cin 128 (256 workgroups: the overlay shape at 76 KB changed nothing end to end)
    {2, 3, 10, 20, 3, 2, 3, 24, 5, false, false, false},  // v2 P3: Cin 48     (v2: any of LITEPI_HEAD_A32 / _2WG / _1WG)
    {2, 6, 10, 10, 2, 1, 6, 24, 5, false, false, false},  // v2 P4: Cin 96
    {2, 12, 8, 8, 1, 1, 6, 24, 5, false, false, false},   // v2 P5: Cin 192
};
constexpr int kNumHeadVariants = (int)(sizeof(kHeadVariants) / sizeof(kHeadVariants[0]));

constexpr const char* head_table_error() {
  for (const HeadVariant& v : kHeadVariants)
    if (v.check()) return v.check();
  return nullptr;
}
static_assert(head_table_error() == nullptr, "kHeadVariants: a row is inconsistent (HeadVariant::check)");

// the profile name: the leading template arguments of head_fused_kernel
inline std::string kernel_name(const HeadVariant& v) {
  char buf[96];
  int n = snprintf(buf, sizeof(buf), "head_fused<%d,%d,%d,%d,%d,%d>", v.c3t, v.pa, v.pb, v.npc(), v.ksa, v.slotf);
  if (v.a16 && v.c3t == 2) snprintf(buf + n, sizeof(buf) - n, "a16k%d", v.kpt);
  else if (v.a16) snprintf(buf + n, sizeof(buf) - n, "a16");
  return buf;
}

// ---- the plan of one level ---------------------------------------------------------------------------------------------
struct HeadPlan {
  bool ok = false;
  const char* plan_err = "not planned";   // why the shape has no plan
  int variant = -1;                       // row of kHeadVariants
  int Cin = 0, c3 = 0, nc = 1;
  int C3T = 1, KPT = 0, TH = 16, TW = 16, PA = 3, PB = 2, NPC = 2, KSA = 6, SLOTF = 24;   // SLOTF: fragments per weight-ring slot
  int OVL = 0;                                  // MID overlays the input tile in LDS
  int A16 = 0;                                  // stage A on 16x16x32 MFMAs (16-pixel tiles)
  int SPLIT_A = 0;                              // A16: class rows of stage A in front of the vote, box rows behind it
  int KSAC = 0, NCAC = 0, KSAB = 0, NCAB = 0;   // its chunks: half-steps per chunk and chunks of the class | box pass
  size_t lds_bytes = 0;
  int nchunks = 0;                              // weight-stream chunks
};

// Cin (physical) -> 64 (c2) box and c3 class channels, nc classes, reg_max DFL bins, under a load's switches.  Everything the
// kernel's shape depends on is checked here: a shape that plans is a shape that packs and launches.
inline HeadPlan plan_head(int cin_phys, int c2, int c3, int nc, int reg_max, const HeadSwitches& sw) {
  HeadPlan p;
  if (c2 != 64 || reg_max != 16 || nc < 1 || nc > 32 || c3 < 8 || c3 > 64 || c3 % 8 != 0 || cin_phys % 16 != 0) {
    p.plan_err = "channel counts outside the fused head's range";
    return p;
  }
  p.Cin = cin_phys; p.c3 = c3; p.nc = nc;
  p.C3T = c3 > 32 ? 2 : 1;
  p.KPT = cin_phys / 16;
  for (int i = 0; i < kNumHeadVariants && p.variant < 0; ++i)
    if (kHeadVariants[i].c3t == p.C3T && kHeadVariants[i].kpt == p.KPT && kHeadVariants[i].selectable(sw)) p.variant = i;
  if (p.variant < 0) {
    p.plan_err = "no kernel configuration for this Cin";
    return p;
  }
  const HeadVariant& v = kHeadVariants[p.variant];
  p.TH = v.th; p.TW = v.tw; p.PA = v.pa; p.PB = v.pb; p.NPC = v.npc(); p.KSA = v.ksa; p.SLOTF = v.slotf;
  p.OVL = v.ov; p.A16 = v.a16; p.SPLIT_A = v.split;
  p.KSAC = v.ksac(); p.NCAC = v.ncac(); p.KSAB = v.ksab(); p.NCAB = v.ncab();
  p.lds_bytes = v.lds_bytes();
  p.nchunks = v.nchunks();
  p.plan_err = v.check();
  p.ok = p.plan_err == nullptr;
  return p;
}

// ---- the weight stream -------------------------------------------------------------------------------------------------
struct Src {  // physical fp32 weights, [out][taps][in]
  const std::vector<float>*wa, *ba;        // merged first convs: [64 + c3][9][Cin], bias [64 + c3]
  const std::vector<float>*wbb, *bbb;      // box tower second conv [64][9][64]
  const std::vector<float>*wpb, *bpb;      // box projection [64][64]
  const std::vector<float>*wbc, *bbc;      // class tower second conv [c3][9][c3]
  const std::vector<float>*wpc, *bpc;      // class projection [ncp][c3] (ncp = physical class channels >= nc)
  int ncp;
};
struct HeadPack {
  std::vector<uint16_t> stream;            // 1 KiB MFMA A fragments in consumption order, every chunk a whole slot image
  std::vector<unsigned short> coff;        // per chunk: first fragment,
  std::vector<unsigned char> csz, cks;     // fragments, K steps
  std::vector<float> biasA, biasB, biasC;  // [32 * RT + 16], [32 * RT + 16], [64 + 32 + 16] (zero padded)
  const char* pack_err = nullptr;          // a chunk that does not fit its slot, or a chunk count that is not the plan's
};

// MFMA row rho of a 32-row tile carries physical channel 16*((rho>>2)&1) + 4*(rho>>3) + (rho&3): the D fragment of lane
// half h then holds channels 16*h .. 16*h+15 in its 16 registers
constexpr int row_channel(int rho) { return 16 * ((rho >> 2) & 1) + 4 * (rho >> 3) + (rho & 3); }

inline HeadPack pack_head(const HeadPlan& p, const Src& s) {
  HeadPack out;
  const int Cin = p.Cin, c3 = p.c3, nc = p.nc, C3T = p.C3T, KPT = p.KPT, KSA = p.KSA, SLOTF = p.SLOTF, RT = 2 + C3T, SPT = (KPT + 1) / 2;
  std::vector<uint16_t>& stream = out.stream;
  auto frag = [&](auto&& weight_of) {  // weight_of(row rho, k element e of the K step) -> float; appends one 1 KiB fragment
    const size_t base = stream.size();
    stream.resize(base + 512);
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) stream[base + lane * 8 + j] = f32_to_f16(weight_of(lane & 31, 8 * (lane >> 5) + j));
  };
  auto begin_chunk = [&]() { out.coff.push_back((unsigned short)(stream.size() / 512)); };
  auto end_chunk = [&](int ksteps) {
    const size_t nf = stream.size() / 512 - out.coff.back();
    if (nf < 1 || (int)nf > SLOTF) out.pack_err = "a chunk does not fit a ring slot";
    out.csz.push_back((unsigned char)nf);
    out.cks.push_back((unsigned char)ksteps);
    stream.resize((size_t)(out.coff.back() + SLOTF) * 512, 0);   // every chunk is a whole slot image
  };
  const std::vector<float>& wa = *s.wa;  // [64 + c3][9][Cin]
  // ---- stage A on 16x16x32 MFMAs: chunk = tap; K step (tap, q) covers input channels 32 q .. 32 q + 31; per K step two half-steps
  //      of RT row tiles (16 rows each).  Fragment lane l: row l & 15 of the tile, K group kg = l >> 4 = channel slot gam(kg) =
  //      {0, 2, 1, 3} of the step's four (the kernel's pixel fragments read the same slot order: conflict-free LDS reads).  Row r
  //      of row tile R (= rh * RT + rt) is physical MID channel 32 (R >> 1) + 8 (r >> 2) + 4 (R & 1) + (r & 3): a lane's D
  //      registers of tiles 2t | 2t+1 are then 8 consecutive channels of one pixel -> one 16-byte MID store.
  auto frag16 = [&](auto&& weight_of) {  // weight_of(row r, k element e of the 32) -> float; appends one 1 KiB fragment
    const size_t base = stream.size();
    stream.resize(base + 512);
    for (int lane = 0; lane < 64; ++lane)
      for (int j = 0; j < 8; ++j) {
        const int kg = lane >> 4, slot = (kg & 1) * 2 + (kg >> 1);
        stream[base + lane * 8 + j] = f32_to_f16(weight_of(lane & 15, 8 * slot + j));
      }
  };
  // one pass of the A16 first convs: RTP row tiles per half-step from row tile R0 on, KPC K steps per chunk
  auto packA16 = [&](int R0, int RTP, int KPC) {
    for (int ks = 0; ks < 9 * SPT; ++ks) {
      const int tap = ks / SPT, q = ks % SPT;
      if (ks % KPC == 0) begin_chunk();
      for (int rh = 0; rh < 2; ++rh)
        for (int rt = 0; rt < RTP; ++rt)
          frag16([&](int r, int e) {
            const int R = R0 + rh * RTP + rt;
            const int c = 32 * (R >> 1) + 8 * (r >> 2) + 4 * (R & 1) + (r & 3);   // physical MID channel
            const int src = c < 64 ? c : (c - 64 < c3 ? 64 + (c - 64) : -1);
            return (src < 0 || 32 * q + e >= Cin) ? 0.f : wa[((size_t)src * 9 + tap) * Cin + 32 * q + e];
          });
      if (ks % KPC == KPC - 1) end_chunk(2 * KPC);
    }
  };
  if (p.A16 && !p.SPLIT_A) packA16(0, RT, KSA / 2);
  if (p.SPLIT_A) packA16(4, C3T, p.KSAC / 2);   // the class rows: row tiles 4 ..; the box rows follow the class projection
  // ---- stage A: K step (tap, cg): element e = input channel 16*cg + e
  for (int ks = 0; ks < (p.A16 ? 0 : 9 * KPT); ++ks) {
    if (ks % KSA == 0) begin_chunk();
    const int tap = ks / KPT, cg = ks % KPT;
    for (int rt = 0; rt < RT; ++rt)
      frag([&](int rho, int e) {
        const int c = rt * 32 + row_channel(rho);          // physical MID channel
        const int src = c < 64 ? c : (c - 64 < c3 ? 64 + (c - 64) : -1);
        return src < 0 ? 0.f : wa[((size_t)src * 9 + tap) * Cin + 16 * cg + e];
      });
    if (ks % KSA == KSA - 1) end_chunk(KSA);
  }
  // ---- stage B class (in front of the box tower: the kernel runs it first): 2*C3T K steps per tap
  {
    const int per_tap = 2 * C3T, total = 9 * per_tap, per_chunk = C3T == 2 ? SLOTF / 2 : (SLOTF >= 18 ? 18 : 6);
    for (int kq = 0; kq < total; ++kq) {
      if (kq % per_chunk == 0) begin_chunk();
      const int tap = kq / per_tap, cg = kq % per_tap;
      for (int rt = 0; rt < C3T; ++rt)
        frag([&](int rho, int e) {
          const int co = rt * 32 + row_channel(rho), ci = 16 * cg + e;
          return (co < c3 && ci < c3) ? (*s.wbc)[((size_t)co * 9 + tap) * c3 + ci] : 0.f;
        });
      if (kq % per_chunk == per_chunk - 1) end_chunk(per_chunk);
    }
  }
  // ---- stage C: K step (mt, s): element e of lane half hh = mid channel 32*mt + 16*hh + 8*s + (e & 7), hh = e >> 3
  auto box_proj = [&]() {
    for (int rt = 0; rt < 2; ++rt)
      for (int q = 0; q < 4; ++q)
        frag([&](int rho, int e) {
          const int mt = q >> 1, sq = q & 1;
          const int ci = 32 * mt + 16 * (e >> 3) + 8 * sq + (e & 7);
          return (*s.wpb)[(size_t)(rt * 32 + row_channel(rho)) * 64 + ci];
        });
  };
  auto cls_proj = [&]() {
    for (int q = 0; q < 2 * C3T; ++q)
      frag([&](int rho, int e) {
        const int mt = q >> 1, sq = q & 1;
        const int ci = 32 * mt + 16 * (e >> 3) + 8 * sq + (e & 7), co = row_channel(rho);
        return (co < nc && ci < c3) ? (*s.wpc)[(size_t)co * c3 + ci] : 0.f;
      });
  };
  // stream order = consumption order: A chunks | class-B chunks | class projection | box-B chunks | box projection (a workgroup
  // whose tile holds no candidate leaves behind the class projection); split stage A: class-A chunks | class-B chunks | class
  // projection | box-A chunks | box-B chunks | box projection
  begin_chunk(); cls_proj(); end_chunk(0);
  if (p.SPLIT_A) packA16(0, 2, p.KSAB / 2);
  // ---- stage B box: K step kq = (tap, cg), 4 per tap
  const int KSB = SLOTF / 2;   // two row tiles per step
  for (int kq = 0; kq < 36; ++kq) {
    if (kq % KSB == 0) begin_chunk();
    const int tap = kq >> 2, cg = kq & 3;
    for (int rt = 0; rt < 2; ++rt)
      frag([&](int rho, int e) { return (*s.wbb)[((size_t)(rt * 32 + row_channel(rho)) * 9 + tap) * 64 + 16 * cg + e]; });
    if (kq % KSB == KSB - 1) end_chunk(KSB);
  }
  begin_chunk(); box_proj(); end_chunk(0);
  if ((int)out.coff.size() != p.nchunks && !out.pack_err) out.pack_err = "the weight stream's chunk count is not the plan's";
  stream.resize(stream.size() + (size_t)2 * SLOTF * 512, 0);   // the ring requests two chunks past the end
  out.biasA.assign(32 * RT + 16, 0.f); out.biasB.assign(32 * RT + 16, 0.f); out.biasC.assign(64 + 32 + 16, 0.f);
  for (int c = 0; c < 64; ++c) {
    out.biasA[c] = (*s.ba)[c];
    out.biasB[c] = s.bbb->empty() ? 0.f : (*s.bbb)[c];
    out.biasC[c] = s.bpb->empty() ? 0.f : (*s.bpb)[c];
  }
  for (int c = 0; c < c3; ++c) { out.biasA[64 + c] = (*s.ba)[64 + c]; out.biasB[64 + c] = s.bbc->empty() ? 0.f : (*s.bbc)[c]; }
  for (int c = 0; c < nc; ++c) out.biasC[64 + c] = s.bpc->empty() ? 0.f : (*s.bpc)[c];
  return out;
}

}  // namespace hplan
}  // namespace lp
