// Configurations, K orders and weight packers of the whole-C2f, stride-2 and one-launch SPPF kernels (c2f_kernels.hip).
// Host-only and pure: no HIP, no allocation on a device, no environment -- a plain C++ compiler builds it, and
// tests/native/c2f_plan_replay.cpp replays it against a recording (tests/golden/c2f_plans.json).  This header is the only place
// that knows the fragment format: the layers of c2f.h ask its predicates, build() is "check supported, pack, upload", launch() an
// index into the for_each_* lists below, which are also what gets instantiated.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "error.h"
#include "f16.h"

namespace lp {

enum { C2F_W_S2 = 0, C2F_W_CV1, C2F_W_A0, C2F_W_B0, C2F_W_A1, C2F_W_B1, C2F_W_CV2, C2F_W_SP1, C2F_W_SP2, C2F_NW };

// Shape key of an instantiated kernel configuration
struct C2fShape {
  int C = 0;      // hidden channels c of the module (cv1 produces 2c, every bottleneck conv is c -> c)
  int NB = 1;     // bottlenecks
  int KA = 0;     // cv1 input channels taken from src0 (0: none)
  int KB = 0;     // cv1 input channels taken from src1
  int UP = 0;     // src0 is half resolution (fused Interp nearest x2)
  int COUT = 0;   // cv2 output channels
  int MODE = 0;   // 0: C2f; 1: stride-2 3x3 entry conv + C2f (whole image per workgroup); 2: entry conv + C2f + SPPF;
                  // -1: C2f without its cv1 (y0 | y1 already in the concat buffer: the stride-2 conv in front ran cv1 as its tail)
  int KS2 = 0;    // input channels of the entry conv
  bool operator==(const C2fShape& o) const {
    return C == o.C && NB == o.NB && KA == o.KA && KB == o.KB && UP == o.UP && COUT == o.COUT && MODE == o.MODE && KS2 == o.KS2;
  }
};

namespace c2fplan {

// fp32 weights of a whole-C2f launch over physical channels (here physical == logical: the supported shapes have no padded segments)
struct C2fSrc {
  const std::vector<float>*cv1 = nullptr, *cv1_b = nullptr;             // [2C][KA + KB]
  const std::vector<float>*a[2] = {nullptr, nullptr}, *a_b[2] = {nullptr, nullptr};  // [C][9][C]
  const std::vector<float>*bb[2] = {nullptr, nullptr}, *bb_b[2] = {nullptr, nullptr};
  const std::vector<float>*cv2 = nullptr, *cv2_b = nullptr;             // [COUT][(2 + NB) C]
  const std::vector<float>*s2 = nullptr, *s2_b = nullptr;               // [XC][9][KS2]
  const std::vector<float>*sp1 = nullptr, *sp1_b = nullptr;             // [C][COUT]
  const std::vector<float>*sp2 = nullptr, *sp2_b = nullptr;             // [COUT][4C]
};

constexpr int cdiv_c(int a, int b) { return (a + b - 1) / b; }
constexpr int min_c(int a, int b) { return a < b ? a : b; }
constexpr int max_c(int a, int b) { return a > b ? a : b; }
// how many K steps of pixel fragments from global memory a 1x1 phase keeps in flight (C2fCfg::DEEP): as many as ~180
// registers of fragments + accumulators allow.  (Measured neutral: cv1 of the c = 24 module at depth 5 instead of 2, and of
// v1's c = 16 FPN module at 3 instead of 2, ran in the same 82 / 46 us -- a K step's 1.3 k cycles are not one exposed round
// trip, the fetch path is busy with the eight waves' streams whatever the depth.  Kept for v2's configurations.)
constexpr int deep_depth(int S, int NT, int PT, bool ldsw) {
  int d = 2;
  for (int t = 3; t <= 6 && t <= S; ++t)
    if ((t * (PT + (ldsw ? 0 : NT)) + (ldsw ? 2 * NT : 0) + NT * PT) * 4 <= 180) d = t;
  return d;
}
// channel tiles (16 output channels each) per block of a wave: in threes where the count allows it -- v2's 48 / 96 / 192
// channels: NT = 3, a lane owns 12 consecutive channels --, else up to four
constexpr int chan_tiles(int ct) { return ct % 3 == 0 ? 3 : min_c(ct, 4); }
// bytes per LDS pixel of a c-channel plane: an odd number of 16-byte slots.  c % 16 != 0 (c = 24: 48 B = 3 slots): no pad at
// all -- the lanes that own the 8 padding rows of the second channel tile skip their stores
constexpr int pix_pitch(int c) { return c % 16 != 0 ? 2 * c : 2 * c + 16; }
// K steps of a 3x3 conv in the general order (k_3x3_general): 9 taps x cin / ksplit / 8 K groups per pass, four groups per step
constexpr int steps_3x3_general(int cin, int ksplit = 1) { return (9 * (cin / ksplit / 8) + 3) / 4; }

// ---- whole-C2f configurations (c2f_kernel).  The first eight parameters are the shape key, in C2fShape's order (tools/pmc_traffic.py
//      and tools/pmc_summarize.py read them by position); TH_: tile rows; AW_: the phases' weights are staged in LDS; NWT_: waves of a
//      tile configuration, 0 = by width
template <int C_, int NB_, int KA_, int KB_, bool UP_, int COUT_, int MODE_, int KS2_, int TH_ = 20, bool AW_ = true, int NWT_ = 0>
struct C2fCfg {
  static constexpr int C = C_, NB = NB_, KA = KA_, KB = KB_, COUT = COUT_, MODE = MODE_, KS2 = KS2_;
  static constexpr bool UP = UP_;
  static constexpr bool PERIMG = MODE_ >= 1;   // the tile is the whole image: no halo recompute, a 1-pixel zero ring
  // MODE -1: the module WITHOUT cv1 -- the launch in front (the stride-2 conv with cv1 as its 1x1 tail, s2lds_kernel) wrote y0 | y1
  // into the concat buffer; y1 (+ halo) is copied into plane 0.  For n = 2 modules cv1 on the halo-4 region was 2x its work.
  static constexpr bool XCV1 = MODE_ == -1;
  // waves per workgroup.  c = 16: four, so that two workgroups (LDS allows it) share a CU at one wave each per SIMD with
  // the whole register file -- two independent workgroups drift out of phase and cover each other's epilogues and waits;
  // eight waves under a 128-register cap spilled in every epilogue
  // whole-image configurations: eight
  // (NWT_: a tile configuration of c < 32 whose LDS allows only ONE workgroup per CU runs eight waves like the wide ones)
  static constexpr int NW = MODE_ >= 1 ? 8 : (NWT_ > 0 ? NWT_ : (C_ >= 32 ? 8 : 4));
  static constexpr int TH = TH_, TW = 20;
  static constexpr int F = PERIMG ? 1 : 2 * NB;  // frame margin around the tile
  static constexpr int LW = TW + 2 * F, LH = TH + 2 * F;
  // general K packing of the 3x3 convs (v2's widths c = 24 / 48: a tap is not a whole number of 32-channel K steps): K group
  // q = 4 s + gam -> (tap q / (c/8), channel group q % (c/8)), a per-lane table of LDS offsets (c3_phase)
  static constexpr bool GK = C % 32 != 0 && C != 16;
  static constexpr bool DEEP = GK || C == 96;   // (v2's configurations: deep_depth)
  static constexpr int PS = pix_pitch(C);
  // c = 16, one bottleneck: plane 0 holds cv1's whole output y0 | y1 (2c channels per pixel), so that cv2's first K step
  // (32 channels) is one plane-0 read and the module's concat buffer is never touched: no global round trip of y0 .. y2
  static constexpr bool Y01 = C == 16 && NB == 1 && MODE_ == 0;
  static constexpr int PS0 = Y01 ? 4 * C + 16 : PS;   // plane 0 pixel pitch
  static constexpr int Y1OFF = Y01 ? 2 * C : 0;       // byte offset of y1 inside a plane-0 pixel
  static constexpr int PLANE0 = LW * LH * PS0, PLANE = LW * LH * PS;
  static constexpr int XC = 2 * C;               // output channels of the entry conv
  // how far each phase's region extends beyond the tile
  static constexpr int e_cv1 = PERIMG ? 0 : 2 * NB;
  static constexpr int e_a(int k) { return PERIMG ? 0 : 2 * (NB - k) - 1; }
  static constexpr int e_b(int k) { return PERIMG ? 0 : 2 * (NB - k) - 2; }
  static constexpr int npt(int e) { return cdiv_c((TH + 2 * e) * (TW + 2 * e), 16); }
  // block shapes (NT channel tiles x PT pixel tiles per wave, CB channel blocks): one round of blocks per phase, two
  // where one would not fit the register file (cap_pt: 20 accumulator tiles a wave can hold, 21 in threes)
  static constexpr int cap_pt(int nt, int pt) { return nt * pt > (nt == 3 ? 21 : 20) ? cdiv_c(pt, 2) : pt; }
  // (whole-image configurations: cv1's fragments are staged in plane 1, which nothing uses before the first bottleneck conv,
  //  and a wave holds every output channel of two pixel tiles -- as the entry conv, see WB_S2)
  static constexpr bool W1_LDS = PERIMG;
  static constexpr int CT1 = 2 * C / 16, NT1 = W1_LDS ? CT1 : chan_tiles(CT1), CB1 = CT1 / NT1,
                       PT1 = W1_LDS ? 2 : cap_pt(NT1, cdiv_c(npt(e_cv1), NW / CB1));
  static constexpr int CTM = cdiv_c(C, 16), NTM = CTM % 3 == 0 ? 3 : min_c(CTM, 2), CBM = CTM / NTM;
  static constexpr int ptm(int e) { return cdiv_c(npt(e), NW / CBM); }
  static constexpr int CT2 = COUT / 16, NT2 = CT2 % 3 == 0 ? 3 : (CT2 >= 2 ? CT2 / 2 : 1), CB2 = CT2 / NT2, PT2 = cap_pt(NT2, cdiv_c(npt(0), NW / CB2));
  static constexpr int PT2W = cdiv_c(npt(0), NW / CB2);   // whole-image cv2: one round of blocks (pw_sync_phase)
  static constexpr int NTS = NTM, CBS = CBM, PTS = cdiv_c(npt(0), NW / CBS);  // SPPF.cv1 (c outputs)
  static constexpr int WPS = 2;   // waves per SIMD the register allocation must allow
  // cv2 reads y_NB and y_{NB+1} from the LDS planes (whole K steps need c >= 32); the earlier segments from the concat buffer
  // cv2's K steps straddle the concat's segments (c = 24 / 48; c = 16 with two bottlenecks: 32 channels of y0 | y1 from the concat
  // buffer, y2 and y3 from the planes): pw_gk_phase's per-lane source table
  static constexpr bool CV2_TAB = GK || (C == 16 && NB == 2);
  static constexpr bool CV2_LDS = C >= 32 || Y01 || CV2_TAB;
  static constexpr int K2G = Y01 ? 0 : (CV2_LDS ? NB * C : (2 + NB) * C);
  // weights staged in LDS (tile configurations): fragment bytes of every phase, in execution order
  static constexpr bool AW = !PERIMG && AW_;
  static constexpr int c3_steps = GK ? steps_3x3_general(C) : (C >= 32 ? 9 * (C / 32) : 5);
  static constexpr int WB_CV1 = CT1 * cdiv_c(KA + KB, 32) * 1024, WB_M = CTM * c3_steps * 1024, WB_CV2 = CT2 * cdiv_c((2 + NB) * C, 32) * 1024;
  static constexpr int WSLOT = AW ? max_c(WB_CV1, max_c(WB_M, WB_CV2)) : 0;
  // whole-image configurations: the entry conv runs before anything lives in the planes, so ALL of its fragments are staged
  // in LDS (144 KB for 64 -> 128 channels) and a wave holds every output channel of its pixels (NT = all row tiles): each
  // pixel fragment is gathered from global memory exactly once per workgroup.  With the weights streamed from L2 by every
  // wave this phase moved 2 MB through the CU's L1 and took 88 k of the kernel's 230 k cycles.
  static constexpr int NT_S2 = XC / 16, PT_S2 = 2;
  static constexpr int WB_S2 = PERIMG ? NT_S2 * 9 * (KS2 / 32) * 1024 : 0;
  static constexpr int LDS_BYTES = max_c(PLANE0 + PLANE + 2 * WSLOT, WB_S2);
  static_assert(!W1_LDS || WB_CV1 <= PLANE, "cv1's fragments are staged in plane 1");
  static C2fShape shape() {
    C2fShape s;
    s.C = C; s.NB = NB; s.KA = KA; s.KB = KB; s.UP = UP ? 1 : 0; s.COUT = COUT; s.MODE = MODE; s.KS2 = KS2;
    return s;
  }
};

// instantiated configurations (YOLO-LitePi v1 widths; model.ncnn.param line of the module's cv1)
typedef C2fCfg<32, 1, 128, 64, true, 64, 0, 0> CfgNeck40;    // :90  up(P5) | P4 -> C2f(n=1) @40x40
typedef C2fCfg<16, 1, 64, 32, true, 32, 0, 0, 16> CfgNeck80;     // :105 up(F4) | P3 -> C2f(n=1) @80x80
typedef C2fCfg<32, 1, 0, 128, false, 64, 0, 0> CfgPan40;     // :121 conv_37 | F4 -> C2f(n=1) @40x40
typedef C2fCfg<64, 1, 0, 256, false, 128, 1, 64> CfgPan20;   // :134-147 conv_42 (s2) | P5 -> C2f(n=1) @20x20
typedef C2fCfg<64, 1, 0, 128, false, 128, 2, 64> CfgBb20;    // :62-85 conv_22 (s2) -> C2f(n=1) -> SPPF @20x20
typedef C2fCfg<16, 2, 0, 32, false, 32, 0, 0, 16> CfgBb80;       // :22-38 C2f(n=2) @80x80
typedef C2fCfg<32, 2, 0, 64, false, 64, 0, 0> CfgBb40;       // :43-59 C2f(n=2) @40x40
// YOLO-LitePi v2 widths (src/tt100k/convert/model/yolo_plus/yolo_plus_ncnn_model/model.ncnn.param, line of the module's cv1).
// c = 48 / 96: the phases' weights do not fit beside the planes -- every wave streams its channel block's fragments from L2 (AW off)
typedef C2fCfg<48, 1, 192, 96, true, 96, 0, 0, 20, false> CfgV2Neck40;   // :101 up(P5) | P4 -> C2f(n=1) @40x40
typedef C2fCfg<48, 1, 0, 144, false, 96, 0, 0, 20, false> CfgV2Pan40;    // :132 conv_37 | F4 -> C2f(n=1) @40x40
typedef C2fCfg<24, 1, 96, 48, true, 48, 0, 0, 16> CfgV2Neck80;           // :116 up(F4) | P3 -> C2f(n=1) @80x80
typedef C2fCfg<96, 1, 0, 192, false, 192, 0, 0, 10, false> CfgV2Bb20;    // :63 C2f(n=1) @20x20, two half-image tiles
typedef C2fCfg<96, 1, 0, 288, false, 192, 0, 0, 10, false> CfgV2Pan20;   // :145 conv_42 | P5 -> C2f(n=1) @20x20, two half-image tiles
typedef C2fCfg<24, 2, 0, 48, false, 48, -1, 0, 20, true, 8> CfgV2Bb80x;  // v2 :13-26 C2f(n=2) @80x80 without cv1 (as CfgBb80x)
typedef C2fCfg<16, 2, 0, 32, false, 32, -1, 0, 16> CfgBb80x;     // v1 :22-38 C2f(n=2) @80x80 WITHOUT cv1 (MODE -1: cv1 is the tail of the stride-2 conv in front)
typedef C2fCfg<64, 1, 0, 256, false, 128, 0, 0, 10, false> CfgPan20h;    // v1's PAN 20x20 module WITHOUT its entry conv on two half-image tiles (A/B:
typedef C2fCfg<64, 1, 0, 128, false, 128, 0, 0, 10, false> CfgBb20h;     //  LITEPI_C2F_SKIP of the whole-image configurations), and the backbone's
typedef C2fCfg<24, 2, 0, 48, false, 48, 0, 0, 20, true, 8> CfgV2Bb80;    // :13 C2f(n=2) @80x80 (halo 4; 103 KB: ONE workgroup per CU, so eight waves
                                                                         // and 20-row tiles: 130 -> 123 -> 119 us; the n = 1 module on the same shape: 91 vs 80 us for two 4-wave workgroups)
typedef C2fCfg<48, 2, 0, 96, false, 96, 0, 0, 10, false> CfgV2Bb40;      // :30 C2f(n=2) @40x40 (halo 4, 10-row tiles)

// the profile name of a shape: "c2f<c,n,src>", src = cv1's K segments ("y0y1": cv1 ran in the launch in front; "s2+": behind the entry conv)
inline std::string c2f_name(const C2fShape& s) {
  const std::string src = s.MODE == -1 ? "y0y1" : (s.MODE >= 1 ? fmt(s.MODE == 2 ? "s2+%d,sppf" : "s2+%d", s.KB) : (s.UP ? fmt("up%d+%d", s.KA, s.KB) : fmt("%d", s.KA + s.KB)));
  return fmt("c2f<%d,%d,%s>", s.C, s.NB, src.c_str());
}

// every instantiated configuration, in one place: f.template operator()<CFG>() until one returns true.  No switches here or in
// the predicates below: which configurations a load may use is the planner's business (PlanSwitches, detector_plan.cpp), and a
// layer that was planned keeps its kernel
// (v2's n = 2 backbone modules run as one launch each: 139 us against 150 for the four launches of the 80x80 one -- 145 before
//  cv2 took y2 / y3 from the planes --, +1.5 % of the pipelined rate; 10-row tiles on the 40x40 map: 74 against 118)
template <class F> bool for_each_cfg(F&& f) {
  return f.template operator()<CfgNeck40>() || f.template operator()<CfgNeck80>() || f.template operator()<CfgPan40>() ||
         f.template operator()<CfgPan20>() || f.template operator()<CfgBb20>() || f.template operator()<CfgBb80>() ||
         f.template operator()<CfgBb40>() || f.template operator()<CfgV2Neck40>() || f.template operator()<CfgV2Pan40>() ||
         f.template operator()<CfgV2Neck80>() || f.template operator()<CfgV2Bb20>() || f.template operator()<CfgV2Pan20>() ||
         f.template operator()<CfgV2Bb80>() || f.template operator()<CfgV2Bb40>() || f.template operator()<CfgPan20h>() ||
         f.template operator()<CfgBb20h>() || f.template operator()<CfgBb80x>() || f.template operator()<CfgV2Bb80x>();
}

// ---- stride-2 configurations.  S2Cfg (s2conv_kernel): the pixel operand gathered from global memory, weights once in LDS
template <int CIN_, int COUT_, int TH_ = 20>
struct S2Cfg {
  static constexpr int KS2 = CIN_, COUT = COUT_, NW = 8, TH = TH_, TW = 20, F = 0, C = 32;
  static constexpr int CT = COUT / 16, NT = chan_tiles(CT), CB = CT / NT, PT = cdiv_c(cdiv_c(TH * TW, 16), NW / CB);
  static constexpr int WBYTES = CT * 9 * (KS2 / 32) * 1024;
  // what the rows (s2_row) read from either stride-2 configuration type, under S2LCfg's names
  static constexpr bool LDS_STAGED = false, TAIL = false;
  static constexpr int CIN = CIN_, OSPLIT = 1, KSPLIT = 1, S = 9 * (KS2 / 32), LDS_BYTES = WBYTES;
};
// S2LCfg (s2lds_kernel): the INPUT tile staged in LDS, general K order in KSPLIT passes, OSPLIT workgroups per output tile
template <int CIN_, int COUT_, int TH_, int OSPLIT_, int KSPLIT_ = 1, bool TAIL_ = false>
struct S2LCfg {
  // TAIL: a 1x1 conv + SiLU on the result (C2f.cv1 behind the stride-2 conv: COUT -> COUT channels) runs on the accumulators --
  // a lane's 4 NT consecutive channels of a pixel ARE a K group of the next MFMA's pixel operand (conv_kernels.hip tail_store)
  static constexpr bool TAIL = TAIL_, LDS_STAGED = true;
  static constexpr int CIN = CIN_, COUT = COUT_, TH = TH_, TW = 20, NW = 8, OSPLIT = OSPLIT_, KSPLIT = KSPLIT_;
  static constexpr int COUTW = COUT / OSPLIT;   // output channels of one workgroup
  static constexpr int CINH = CIN / KSPLIT;     // input channels of one pass (Cin 96: two passes of 48 -- a 21 x 41 plane of 96 is 179 KB)
  static constexpr int CT = COUTW / 16, NT = chan_tiles(CT), CB = CT / NT;
  static constexpr bool GK = CINH % 32 != 0;
  static constexpr int G = CINH / 8, S = GK ? cdiv_c(9 * G, 4) : 9 * (CINH / 32);   // K groups per tap, K steps per pass
  static_assert(S == steps_3x3_general(CIN, KSPLIT), "the kernel's K steps per pass are those of k_3x3_general");
  static constexpr int IH = 2 * TH + 1, IW = 2 * TW + 1, LW = IW;
  static constexpr int PS = pix_pitch(CINH);
  static constexpr int PLANE = ((IH * LW * PS + 1023) / 1024) * 1024, WBYTES = CT * S * 1024, LDS_BYTES = PLANE + WBYTES;
  static constexpr int NPT = cdiv_c(TH * TW, 16), PT = cdiv_c(NPT, NW / CB), NBLK = cdiv_c(NPT, PT) * CB;
  static_assert(COUT % (16 * OSPLIT) == 0 && COUTW % (16 * NT) == 0 && NW % CB == 0 && CIN % (8 * KSPLIT) == 0 && LDS_BYTES <= 160 * 1024 && NBLK <= NW,
                "s2lds: shape (one block per wave: the accumulators live across the passes)");
  static_assert(CB == 1 || KSPLIT == 1, "the packed weights are [channel block][all K steps]: a pass is contiguous only for one block");
  // (NT = 2: a lane's 8 channels are one K group, one K step; NT = 3: its 12 channels are K group g of step 0 and the first half of
  //  K group g of step 1, whose second half is zero -- the tail's weights are packed to that order, k_tail)
  static constexpr int TSTEPS = NT == 3 ? 2 : 1;
  static_assert(!TAIL || (OSPLIT == 1 && CB == 1 && ((NT == 2 && COUT == 32) || (NT == 3 && COUT == 48))), "tail: the workgroup holds every channel of a pixel");
};
typedef S2LCfg<24, 48, 10, 1> S2L24x48;   // yolo_plus model.ncnn.param:10 (conv_8: 24 -> 48 @80x80): 41 KB plane + 21 KB of weights
// (Cin 48 in two passes of 24 input channels: 41 KB plane + 21 KB of weights, two workgroups per CU.  The one-pass forms -- 96 KB plane +
//  42 KB -- lost)
typedef S2LCfg<48, 96, 10, 2, 2> S2L48x96k2;   // :27 (conv_15: 48 -> 96 @40x40), two workgroups per tile
typedef S2LCfg<48, 48, 10, 1, 2> S2L48x48k2;   // :129 (conv_37: 48 -> 48 @40x40)
// (v1's 32 -> 64 convs as S2LCfg<32, 64, 10, 1, 2>, two passes of 16 channels: 22.9 / 16.2 us against 22.0 / 14.0 for the gather kernel
//  -- at Cin 32 the tile copy costs what the gathers cost; they stay on s2conv_kernel)
typedef S2LCfg<16, 32, 10, 1, 1, true> S2L16x32t;   // v1 model.ncnn.param:19-20 (conv_6 16 -> 32 @80x80 + conv_7 = C2f.cv1 32 -> 32 as its tail)
typedef S2LCfg<24, 48, 10, 1, 1, true> S2L24x48t;   // v2 :10-11 (conv_8 24 -> 48 @80x80 + conv_9 = C2f.cv1 48 -> 48 as its tail)
typedef S2LCfg<64, 128, 10, 2, 2> S2L64x128;   // v1's 64 -> 128 convs @20x20 (model.ncnn.param:62, :134) when they do not ride in the whole-image kernels
typedef S2LCfg<96, 192, 10, 4, 2> S2L96x192;   // :44 (conv_22: 96 -> 192 @20x20): two passes of 48 input channels, four workgroups per tile
typedef S2LCfg<96, 96, 10, 2, 2> S2L96x96;     // :142 (conv_42: 96 -> 96 @20x20)
typedef S2Cfg<32, 64> S2Cfg32x64;   // model.ncnn.param:41 (conv_15: 32 -> 64 @40x40) and :118 (conv_37)

// every instantiated stride-2 configuration in one place, as for_each_cfg.  The key of an entry is (CIN, COUT, TAIL) of the type
// itself; supported, build and launch are lookups, so a shape cannot be in one and not in another.
template <class F> bool for_each_s2cfg(F&& f) {
  return f.template operator()<S2L24x48>() || f.template operator()<S2L48x96k2>() || f.template operator()<S2L48x48k2>() ||
         f.template operator()<S2L64x128>() || f.template operator()<S2L96x192>() || f.template operator()<S2L96x96>() ||
         f.template operator()<S2L16x32t>() || f.template operator()<S2L24x48t>() || f.template operator()<S2Cfg32x64>();
}

// ---- SPPF in one launch (sppf_kernel): one plane of C channels over the whole image, OSPLIT workgroups per image.  One
//      instantiated configuration; supported / pack / launch read this type only
template <int C_, int CIN_, int COUT_, int OSPLIT_>
struct SpCfg {
  static constexpr int C = C_, CIN = CIN_, COUT = COUT_, OSPLIT = OSPLIT_, COUTW = COUT / OSPLIT, NW = 8, TH = 20, TW = 20, F = 0, LW = 20;
  static constexpr int PS = pix_pitch(C);
  static constexpr bool PERIMG = false, DEEP = true;
  static constexpr int NT1 = chan_tiles(C / 16), CB1 = C / 48, PT1 = cdiv_c(25, NW / CB1);
  static constexpr int NT2 = chan_tiles(COUTW / 16), CB2 = COUTW / 48, PT2 = cdiv_c(25, NW / CB2);
  static constexpr int SPT = C / 32, LDS_BYTES = TH * TW * PS;
  static_assert(C % 96 == 0 && CIN % 32 == 0 && COUTW % 48 == 0 && NW % CB1 == 0 && NW % CB2 == 0 && CB2 * cdiv_c(25, PT2) <= NW && NT2 * PT2 <= 28,
                "sppf: shape (one block per wave in cv2: the accumulators live across the pools)");
};
typedef SpCfg<96, 192, 192, 2> SpCfgV2;   // yolo_plus model.ncnn.param:75-87 (conv_27, three pools, conv_28): 83 KB plane, two workgroups per image
typedef SpCfgV2 SppfCfg;

// ---- one row per instantiation: what the host needs of a configuration type, as values
struct C2fRow {
  std::string name;   // profile name
  C2fShape key;
  int th, tw, waves, lds_bytes, wg_per_tile;
  int nt1, ntm, nt2, nt_s2;   // channel tiles per block of cv1, the 3x3 convs (and SPPF.cv1), cv2 (and SPPF.cv2), the entry conv
  bool perimg, gk, cv2_lds;
};
struct S2Row {
  std::string name;
  int cin, cout;
  bool tail;   // (cin, cout, tail): the key
  int th, tw, waves, lds_bytes, wg_per_tile;
  int nt, ksplit, S;   // channel tiles per block, passes over the input channels, K steps per pass
  bool lds_staged;     // s2lds_kernel (input tile in LDS, general K order in ksplit passes); else s2conv_kernel (gather, cin % 32 == 0 order)
};
struct SppfRow {
  std::string name;
  int cin, c, cout;   // the key
  int th, tw, waves, lds_bytes, wg_per_tile;
  int nt1, nt2;
};
template <class CFG> C2fRow c2f_row() {
  return C2fRow{c2f_name(CFG::shape()), CFG::shape(), CFG::TH, CFG::TW, CFG::NW, CFG::LDS_BYTES, 1, CFG::NT1, CFG::NTM, CFG::NT2, CFG::NT_S2, CFG::PERIMG, CFG::GK,
                CFG::CV2_LDS};
}
inline std::string s2_name(int cin, int cout, bool tail) { return fmt(tail ? "s2conv+1x1<%d,%d>" : "s2conv<%d,%d>", cin, cout); }
template <class CFG> S2Row s2_row() {
  return S2Row{s2_name(CFG::CIN, CFG::COUT, CFG::TAIL), CFG::CIN, CFG::COUT, CFG::TAIL, CFG::TH, CFG::TW, CFG::NW, CFG::LDS_BYTES, CFG::OSPLIT, CFG::NT,
               CFG::KSPLIT, CFG::S, CFG::LDS_STAGED};
}
inline std::string sppf_name(int cin, int c, int cout) { return fmt("sppf<%d,%d,%d>", cin, c, cout); }
inline SppfRow sppf_row() {
  typedef SppfCfg CFG;
  return SppfRow{sppf_name(CFG::CIN, CFG::C, CFG::COUT), CFG::CIN, CFG::C, CFG::COUT, CFG::TH, CFG::TW, CFG::NW, CFG::LDS_BYTES, CFG::OSPLIT, CFG::NT1, CFG::NT2};
}
struct C2fRowsFn {
  std::vector<C2fRow>& v;
  template <class CFG> bool operator()() const { v.push_back(c2f_row<CFG>()); return false; }
};
struct S2RowsFn {
  std::vector<S2Row>& v;
  template <class CFG> bool operator()() const { v.push_back(s2_row<CFG>()); return false; }
};
// the tables, in the order of the for_each_* lists: row i is what launch() reaches as the list's i-th type
inline const std::vector<C2fRow>& c2f_rows() {
  static const std::vector<C2fRow> rows = [] { std::vector<C2fRow> v; for_each_cfg(C2fRowsFn{v}); return v; }();
  return rows;
}
inline const std::vector<S2Row>& s2_rows() {
  static const std::vector<S2Row> rows = [] { std::vector<S2Row> v; for_each_s2cfg(S2RowsFn{v}); return v; }();
  return rows;
}
inline const C2fRow* find_c2f(const C2fShape& s) {
  for (const C2fRow& r : c2f_rows())
    if (r.key == s) return &r;
  return nullptr;
}
inline const S2Row* find_s2(int cin, int cout, bool tail) {
  for (const S2Row& r : s2_rows())
    if (r.cin == cin && r.cout == cout && r.tail == tail) return &r;
  return nullptr;
}

// ---- pure predicates over the rows (the members of c2f.h's layers are one-line calls of these)
inline bool c2f_supported(const C2fShape& s, int h, int w) {
  const C2fRow* r = find_c2f(s);
  if (!r || h % r->th != 0 || w % r->tw != 0) return false;
  if (r->perimg && (h != r->th || w != r->tw)) return false;
  if (s.UP && (h % 2 || w % 2)) return false;
  return r->lds_bytes <= 160 * 1024;
}
inline std::string c2f_kernel_name(const C2fShape& s) {   // "c2f<..>", or empty: no configuration for this shape
  const C2fRow* r = find_c2f(s);
  return r ? r->name : "";
}
inline bool c2f_cv2_from_lds(const C2fShape& s) {
  const C2fRow* r = find_c2f(s);
  return r && r->cv2_lds;
}
inline bool s2_fits(int cin, int cout, bool tail, int hout, int wout) {
  const S2Row* r = find_s2(cin, cout, tail);
  return r && hout % r->th == 0 && wout % r->tw == 0;
}
inline bool s2_supported(int cin, int cout, int hout, int wout) { return s2_fits(cin, cout, false, hout, wout); }
inline bool s2_tail_supported(int cin, int cout, int cout2, int hout, int wout) { return cout2 == cout && s2_fits(cin, cout, true, hout, wout); }
inline bool s2_lds_staged(int cin, int cout) {
  const S2Row* r = find_s2(cin, cout, false);
  return r && r->lds_staged;
}
inline bool sppf_supported(int cin, int c, int cout, int h, int w) {
  return cin == SppfCfg::CIN && c == SppfCfg::C && cout == SppfCfg::COUT && h == SppfCfg::TH && w == SppfCfg::TW;
}

// ---- K orders of the packed A fragments, each named once: (K step s, lane group g, element j) -> index into a row of the weight
//      matrix, or -1 (zero).  A lane group holds K group gam(g) of its step (the LDS column permutation, top of c2f_kernels.hip).
inline int gam_of(int g) { return ((g & 1) << 1) | (g >> 1); }
// 1x1: the row's ktot channels in order
inline auto k_1x1(int ktot) {
  return [ktot](int s, int g, int j) {
    const int k = 32 * s + 8 * gam_of(g) + j;
    return k < ktot ? k : -1;
  };
}
// 3x3, rows [tap][cin], general order (C2fCfg::GK, S2LCfg): K group q = 4 s + gam -> (tap q / G, channel group q % G) over the
// G = cin / ksplit / 8 groups of one pass; the steps of pass h (input channels h cin / ksplit ..) follow those of pass h - 1
inline auto k_3x3_general(int cin, int ksplit = 1) {
  const int cinh = cin / ksplit, G = cinh / 8, S = steps_3x3_general(cin, ksplit);
  return [=](int s, int g, int j) {
    const int h = s / S, q = 4 * (s % S) + gam_of(g);
    return q < 9 * G ? (q / G) * cin + h * cinh + 8 * (q % G) + j : -1;
  };
}
// 3x3, cin % 32 == 0: K step s -> (tap s / (cin / 32), 32-channel block s % (cin / 32))
inline auto k_3x3_c32(int cin) {
  const int spt = cin / 32;
  return [=](int s, int g, int j) { return (s / spt) * cin + 32 * (s % spt) + 8 * gam_of(g) + j; };
}
// 3x3, 16 channels: a K step covers two taps (TA for the even lane groups, TB for the odd ones), five steps
inline auto k_3x3_c16(int cin) {
  return [=](int s, int g, int j) {
    static const int TA[5] = {0, 3, 6, 1, 4}, TB[5] = {2, 5, 8, 7, -1};
    const int tap = (g & 1) ? TB[s] : TA[s];
    return tap < 0 ? -1 : tap * cin + 8 * (g >> 1) + j;
  };
}
// the 1x1 tail of a stride-2 launch: its K groups follow the lanes' channel ownership -- lane group g holds channels
// 4 NT g .. 4 NT (g + 1) - 1 of its pixel, eight per K step (S2LCfg::TSTEPS; NT = 3: the second step's upper half is zero)
inline auto k_tail(int nt) {
  const int own = 4 * nt;
  return [own](int s, int g, int j) { return 8 * s + j < own ? own * g + 8 * s + j : -1; };
}

// A fragments of one phase: [channel block][K step][tile][lane][8 halfs]; lane (g = lane >> 4, m = lane & 15) holds
// A[row m][K group g].  Rows are permuted so that a lane's D rows 4g .. 4g+3 of tiles 0 .. NT-1 are 4*NT consecutive
// channels (vector stores).  kidx(s, g, j) -> index into the K axis of Wm ([cout][ktot]) or -1 (zero).
template <class KIDX>
std::vector<uint16_t> pack_phase(const std::vector<float>& Wm, int cout, int ktot, int NT, int S, KIDX&& kidx) {
  LP_CHECK((int)Wm.size() == cout * ktot, LP_ERR_STATE, "c2f: weight matrix %zu != %d x %d", Wm.size(), cout, ktot);
  const int CB = (cout + 16 * NT - 1) / (16 * NT);   // (rows past cout: the zero padding of the last channel tile)
  std::vector<uint16_t> buf((size_t)CB * S * NT * 64 * 8, 0);
  for (int cb = 0; cb < CB; ++cb)
    for (int s = 0; s < S; ++s)
      for (int t = 0; t < NT; ++t)
        for (int lane = 0; lane < 64; ++lane) {
          const int g = lane >> 4, m = lane & 15, gm = m >> 2, r = m & 3;
          const int oc = cb * 16 * NT + gm * 4 * NT + t * 4 + r;
          const size_t f = ((((size_t)cb * S + s) * NT + t) * 64 + lane) * 8;
          if (oc >= cout) continue;
          for (int j = 0; j < 8; ++j) {
            const int k = kidx(s, g, j);
            if (k >= 0) buf[f + j] = f32_to_f16(Wm[(size_t)oc * ktot + k]);
          }
        }
  return buf;
}
// fp32 bias in natural channel order, zero padded (the last block's lanes read past cout)
inline std::vector<float> pad_bias(const std::vector<float>* b, int cout) {
  std::vector<float> v(cout + 64, 0.f);
  if (b) {
    LP_CHECK((int)b->size() >= cout, LP_ERR_STATE, "c2f: bias vector too short");
    for (int c = 0; c < cout; ++c) v[c] = (*b)[c];
  }
  return v;
}
inline std::vector<uint16_t> pack_1x1(const std::vector<float>& wv, int cout, int ktot, int NT) {
  return pack_phase(wv, cout, ktot, NT, (ktot + 31) / 32, k_1x1(ktot));
}
// 3x3 weights [cout][tap][cin] in the order c3_phase / c3s2_phase read them at this width
inline std::vector<uint16_t> pack_3x3(const std::vector<float>& wv, int cout, int cin, int NT) {
  if (cin % 32 != 0 && cin != 16) return pack_phase(wv, cout, 9 * cin, NT, steps_3x3_general(cin), k_3x3_general(cin));
  if (cin >= 32) return pack_phase(wv, cout, 9 * cin, NT, 9 * (cin / 32), k_3x3_c32(cin));
  return pack_phase(wv, cout, 9 * cin, NT, 5, k_3x3_c16(cin));
}

// ---- the three packers: what build() uploads, as host vectors (an empty vector: the launch does not use the slot)
struct C2fPack {
  std::vector<uint16_t> w[C2F_NW];   // MFMA A fragments per phase
  std::vector<float> b[C2F_NW];      // fp32 bias per phase
  int lds_bytes = 0;
  double macs_per_image = 0;
};
inline C2fPack pack_c2f(const C2fShape& s, int h, int w, const C2fSrc& src) {
  const C2fRow* r = find_c2f(s);
  LP_CHECK(r, LP_ERR_STATE, "c2f: no configuration for this shape");
  C2fPack p;
  p.lds_bytes = r->lds_bytes;
  const int C = s.C, K1 = s.KA + s.KB, K2 = (2 + s.NB) * C;
  if (s.MODE != -1) {   // (MODE -1: cv1 belongs to the launch in front)
    p.w[C2F_W_CV1] = pack_1x1(*src.cv1, 2 * C, K1, r->nt1);
    p.b[C2F_W_CV1] = pad_bias(src.cv1_b, 2 * C);
  }
  for (int k = 0; k < s.NB; ++k) {
    p.w[C2F_W_A0 + 2 * k] = pack_3x3(*src.a[k], C, C, r->ntm);
    p.b[C2F_W_A0 + 2 * k] = pad_bias(src.a_b[k], C);
    p.w[C2F_W_B0 + 2 * k] = pack_3x3(*src.bb[k], C, C, r->ntm);
    p.b[C2F_W_B0 + 2 * k] = pad_bias(src.bb_b[k], C);
  }
  p.w[C2F_W_CV2] = pack_1x1(*src.cv2, s.COUT, K2, r->nt2);
  p.b[C2F_W_CV2] = pad_bias(src.cv2_b, s.COUT);
  p.macs_per_image = ((s.MODE != -1 ? (double)2 * C * K1 : 0.0) + (double)s.NB * 2 * 9 * C * C + (double)s.COUT * K2) * h * w;
  if (s.MODE >= 1) {
    p.w[C2F_W_S2] = pack_3x3(*src.s2, 2 * C, s.KS2, r->nt_s2);   // NT_S2: every row tile in one wave
    p.b[C2F_W_S2] = pad_bias(src.s2_b, 2 * C);
    p.macs_per_image += 9.0 * s.KS2 * 2 * C * h * w;
  }
  if (s.MODE == 2) {
    p.w[C2F_W_SP1] = pack_1x1(*src.sp1, C, s.COUT, r->ntm);
    p.b[C2F_W_SP1] = pad_bias(src.sp1_b, C);
    p.w[C2F_W_SP2] = pack_1x1(*src.sp2, s.COUT, 4 * C, r->nt2);
    p.b[C2F_W_SP2] = pad_bias(src.sp2_b, s.COUT);
    p.macs_per_image += ((double)C * s.COUT + (double)s.COUT * 4 * C) * h * w;
  }
  return p;
}

// stride-2 conv, weights [cout][tap][cin]; w_tail [cout][cout] (1x1), b_tail: the fused tail, or null
struct S2Pack {
  std::vector<uint16_t> w, w2;
  std::vector<float> b, b2;
};
inline S2Pack pack_s2(int cin, int cout, const std::vector<float>& w_taps, const std::vector<float>& bias, const std::vector<float>* w_tail,
                      const std::vector<float>* b_tail) {
  const S2Row* r = find_s2(cin, cout, w_tail != nullptr);
  LP_CHECK(r, LP_ERR_STATE, "s2conv: no configuration for %d -> %d", cin, cout);
  S2Pack p;
  // the row's NT channel tiles per block and K steps.  LDS-staged: the general order in its KSPLIT passes (Cin 96: two passes of 48
  // input channels, the second pass's steps behind the first's); the gather kernel: whole 32-channel blocks per tap
  if (r->lds_staged) p.w = pack_phase(w_taps, cout, 9 * cin, r->nt, r->ksplit * r->S, k_3x3_general(cin, r->ksplit));
  else p.w = pack_phase(w_taps, cout, 9 * cin, r->nt, r->S, k_3x3_c32(cin));
  p.b = pad_bias(&bias, cout);
  if (w_tail) {
    p.w2 = pack_phase(*w_tail, cout, cout, r->nt, (4 * r->nt + 7) / 8, k_tail(r->nt));
    p.b2 = pad_bias(b_tail, cout);
  }
  return p;
}

// SPPF: w1 [c][cin], w2 [cout][4 c] over physical channels, fp32
struct SppfPack {
  std::vector<uint16_t> w1, w2;
  std::vector<float> b1, b2;
  double macs_per_image = 0;
};
inline SppfPack pack_sppf(int cin, int c, int cout, int h, int w, const std::vector<float>& w1, const std::vector<float>& b1,
                          const std::vector<float>& w2, const std::vector<float>& b2) {
  SppfPack p;
  p.w1 = pack_1x1(w1, c, cin, SppfCfg::NT1);
  p.b1 = pad_bias(&b1, c);
  p.w2 = pack_1x1(w2, cout, 4 * c, SppfCfg::NT2);
  p.b2 = pad_bias(&b2, cout);
  p.macs_per_image = ((double)c * cin + (double)cout * 4 * c) * h * w;
  return p;
}

}  // namespace c2fplan
}  // namespace lp
