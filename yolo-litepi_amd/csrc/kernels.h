// Host launchers of the non-convolution kernels (misc_kernels.hip, post_kernels.hip,
// cls_kernels.hip).  All launches are asynchronous on the given stream.
#pragma once
#include "common.h"
#include "letterbox_core.h"
#include "surface_plan.h"

namespace lp {

// ---- per-image geometry (letterbox + un-letterbox), device resident ------------------
struct ImgGeom {
  long src_off;        // byte offset of this image in the source buffer (uint8 BGR HxWx3)
  int h, w;            // original size
  int new_w, new_h;    // resized (unpadded) size inside the letterboxed square
  int top, left;       // integer border offsets (e2e.py:82-83)
  float ratio;         // r (e2e.py:72)
  float pad_w, pad_h;  // float half pads dw, dh (e2e.py:76-77), subtracted un-rounded in postprocess
};

// ---- misc_kernels.hip ------------------------------------------------------------------
// letterbox (e2e.py:66-86): B images -> uint8 BGR [B,SH,SW,3], cv2.INTER_LINEAR fixed point, border 114.  host_geoms (the B
// geometries) sizes the tiled kernel's LDS rows (lb_row_cap); without them, or when the rows do not fit, the per-pixel kernel runs
void launch_letterbox(const uint8_t* src, const ImgGeom* geom, uint8_t* dst, int B, int SH, int SW, hipStream_t st,
                      const ImgGeom* host_geoms = nullptr);
// Interp nearest x2 (model.ncnn.param:88,103)
void launch_upsample2x(int prec, const View& in, const View& out, int N, hipStream_t st);
// SPPF: three cascaded 5x5/s1/p2 max pools (model.ncnn.param:79-83) in one pass
void launch_sppf_pool(int prec, const View& in, const View& o1, const View& o2, const View& o3, int N, hipStream_t st);
// fallbacks for graphs whose concat/add could not be fused
void launch_add(int prec, const View& a, const View& b, const View& out, int N, hipStream_t st);
void launch_copy(int prec, const View& in, const View& out, int N, hipStream_t st);
// YOLO11: ConvolutionDepthWise 3x3/s1/p1 (+bias, optional SiLU), w fp32 [9][C] over physical channels
void launch_dwconv3x3_act(int prec, const View& in, const View& out, const float* w, const float* bias, int act, int N, hipStream_t st);
// YOLO11 C2PSA attention block (Reshape .. MatMul .. Softmax .. MatMul .. + depthwise positional encoding), see misc_kernels.hip
void launch_psa_attention(int prec, const View& qkv, const View& out, const float* pe_w, const float* pe_b, int heads, int dk, int dv,
                          float scale, int N, hipStream_t st);

// ---- post_kernels.hip -----------------------------------------------------------------
struct Cand {  // one candidate / kept box, 32 bytes
  float x1, y1, x2, y2, score;
  int cls, anchor, pad;
};

struct DecodeLevel {
  const void* box;  // [N,H,W,4*reg_max] view base
  const void* cls;  // [N,H,W,nc] view base
  int box_pitch, cls_pitch, H, W, anchor_off;
};

struct DecodeArgs {
  DecodeLevel lv[4];
  int nlevels, A, nc, reg_max;
  const float* anchors;  // [2][A] grid units (x row, y row)
  const float* strides;  // [A]
  const float* dfl_w;    // [reg_max]
  float* out0;           // optional [N,4+nc,A]
  const ImgGeom* geom;   // [N]
  Cand* cand;            // [N][A]
  int* cand_count;       // [N]
  float conf;
};
// Detect head decode (model.ncnn.param:184-208) + conf filter / xywh->xyxy / un-letterbox /
// clip (e2e.py:255-278) fused; out0 is only written when requested (parity hook).
void launch_decode(int prec, const DecodeArgs& a, int N, hipStream_t st);
// Same filter/transform applied to an existing out0 tensor [N,4+nc,A] (tests).
void launch_filter_out0(const float* out0, int nc, int A, const ImgGeom* geom, Cand* cand, int* cand_count,
                        float conf, int N, hipStream_t st);

// ROI bookkeeping across the batch: every image's NMS block appends its kept ROIs to one list
struct RoiTable {
  int* base;      // [N+1] (unused by the fused path; kept for the host-filled table of lp_classify)
  int* total;     // [2]  min(sum, max_rois), then the unclamped sum
  int* img;       // [max_rois] image index of ROI r
  int* slot;      // [max_rois] detection slot of ROI r within its image
  int* work;      // [2] accumulator + ticket of the NMS blocks (zero between calls)
};

// what the image NMS and the frame NMS of views share (nms_dev.h): results, limits, the ROI rule and the ROI list
struct NmsCommon {
  lp_det* dets;           // [N][max_det]
  int* counts;            // [3N]: kept-after-filter, kept-before-filter, float bits of the mean score before the filter
  int* rects;             // [N][max_det][4] int ROI rectangles of the kept boxes
  int A, max_det, nc;
  float iou;
  int min_area;           // < 0: no ROI filter (lp_detect semantics)
  RoiTable tab;           // tab.total == nullptr: no ROI list
  int max_rois;
  int roi_rule;           // 0: e2e.py:465-473, 1: e2e_optimize.py:480-497 (lp_config::numerics)
  int no_small;           // A/B + tests (LITEPI_NMS_NO_SMALL=1): every image takes the general path
};
// no_small as a launch sees it: set in the arguments or by LITEPI_NMS_NO_SMALL
int nms_no_small(int no_small);

struct NmsArgs {
  const Cand* cand;       // [N][A]
  int* cand_count;        // [N]   (reset to 0 by the kernel for the next call)
  Cand* sorted;           // [N][A] scratch
  const ImgGeom* geom;    // [N]
  NmsCommon c;            // per image
};
// per-class greedy NMS (e2e.py:89-119,280-296) + ROI clip / area filter (e2e.py:465-473) + the batch's ROI list
void launch_nms(const NmsArgs& a, int N, hipStream_t st);
size_t nms_lds_bytes(int A);


// ---- tile_kernels.hip (tiled inference of large frames) -------------------------------------
// crop views slot0 .. slot0+nslots-1 of the view batch [V,S,S,3]: frame[-top : -top+S, -left : -left+S], 114 off the frame
void launch_crop_views(const uint8_t* src, const ImgGeom* geom, uint8_t* dst, int slot0, int nslots, int S, hipStream_t st);

// Scaled views (lp_run_views*): one window view of the view batch, device resident.  The view is the letterbox of
// frame[y : y + h, x : x + w], a frame whose rows are `pitch` bytes apart; no byte outside the frame's frame_bytes is read.
struct ViewWin {
  long src_off;        // byte offset of the FRAME in the source buffer
  long frame_bytes;    // rows * pitch
  int pitch;           // frame row bytes
  int x, y, w, h;      // source window in frame pixels
  int new_w, new_h;    // resized (unpadded) window inside the S x S view
  int top, left;       // integer border offsets
  int pad;
};
// what the letterbox core (letterbox_core.h) resamples: a whole image of the source buffer, the window of a view
LP_LB_HD LbSource lb_source(const uint8_t* src, const ImgGeom& g) { return LbSource{src + g.src_off, (long)g.h * g.w * 3, 3 * g.w, 0, 0, g.w, g.h}; }
LP_LB_HD LbSource lb_source(const uint8_t* src, const ViewWin& v) { return LbSource{src + v.src_off, v.frame_bytes, v.pitch, v.x, v.y, v.w, v.h}; }
template <class Table> LP_LB_HD LbPlace lb_place(const Table& t) { return LbPlace{t.new_w, t.new_h, t.top, t.left}; }
// window views slot0 .. slot0+n-1 of the view batch [V,S,S,3] from wins[0 .. n); host_wins (the same n entries) sizes the
// LDS rows (lb_row_cap): when they do not fit (lb_rows_fit: down-scales beyond ~10x) the per-pixel kernel runs
void launch_window_views(const uint8_t* src, const ViewWin* wins, uint8_t* dst, int slot0, int n, int S, hipStream_t st,
                         const ViewWin* host_wins);

// ---- map_kernels.hip (mapped views, include/litepi.h lp_map_*) ------------------------------
// One mapped view of the view batch, device resident, data of the step as ViewWin is: the view shows the H x W frame at
// frame_off of the source buffer through the table fixed[S][S][2] (view_map.h).
struct MapSlot {
  const int32_t* fixed;
  long frame_off;
  int H, W;
};
// mapped views slot0 .. slot0+n-1 of the view batch [V,S,S,3] through maps[0 .. n) (view_map.h's pixel rule); no byte outside
// a frame's H * W * 3 is read
void launch_map_views(const uint8_t* src, const MapSlot* maps, uint8_t* dst, int slot0, int n, int S, hipStream_t st);
// the boxes of the candidates of slots slot0 .. slot0+n-1 (cand [.][A], their counts read on the device) from view to frame
// coordinates through maps[0 .. n) (view_map.h's box rule), in place
void launch_map_candidates(const MapSlot* maps, Cand* cand, const int* cand_count, int slot0, int n, int A, int S, hipStream_t st);

struct TileFrame { int view0, nviews; };   // frame f's views: vslot[view0 .. view0 + nviews), in the frame's view order
struct FrameNmsArgs {
  Cand* cand;             // [V][A] per-view candidates; after the view sort, frame f's merged list at cand + view0 * A
  int* cand_count;        // [V]   (reset to 0 by the view sort for the next call)
  int* vcnt;              // [V]   candidates per view slot (written by the view sort)
  Cand* sorted;           // [V][A] per-view sorted candidates
  const TileFrame* frames;  // [F]
  const int* vslot;       // [V]   view batch slot of the frames' views, frame-major
  const ImgGeom* fgeom;   // [F] frame geometry (size, src_off)
  NmsCommon c;            // per frame; iou holds the resolved threshold of lp_set_view_merge
  int metric, mode;       // lp_match / lp_merge (lp_set_view_merge); 0, 0 = the reference's rule
};
// per-view sort (one workgroup per view slot, V slots), then the merged per-class greedy NMS of every frame (one workgroup
// per frame; max_views bounds the views of one frame: it sizes the LDS flag masks)
void launch_view_sort(const FrameNmsArgs& a, int V, hipStream_t st);
void launch_frame_nms(const FrameNmsArgs& a, int F, int max_views, hipStream_t st);
// LDS of the frame NMS's two flag masks (removed, kept) for a union of at most max_union candidates; FRAME_NMS_LDS_CAP bounds it,
// i.e. one frame may hold at most about 614 k candidate slots (views x anchors): 73 views of 8400 anchors
size_t frame_nms_lds_bytes(int max_union);
#define FRAME_NMS_LDS_CAP (150 * 1024)

// PIL Image.resize((S,S), BILINEAR) of every ROI + BGR->RGB (e2e.py:385-389): uint8 RGB [R,S,S,3]
struct RoiResizeArgs {
  const uint8_t* src;       // source images
  const ImgGeom* geom;      // per image (src_off/h/w)
  const int* rects;         // [N][max_det][4]
  RoiTable tab;
  uint8_t* out;             // [max_rois,S,S,3]
  int max_det, S;
  int linear;               // 0: PIL bilinear with antialias (e2e.py:366-370, 387), 1: cv2.resize INTER_LINEAR (e2e_optimize.py:388-390)
};
// one launch, four (ROI, 16-row strip) units per ROI over a grid of the device's resident workgroups; max_items bounds the ROI count
void launch_roi_resize(const RoiResizeArgs& a, int max_items, hipStream_t st);

// ---- csc_kernels.hip (NV12 frames -> the packed BGR frames the pipeline reads) ---------------
struct CscFrame {      // one frame of a conversion call, device resident
  long src_off;        // byte offset of the frame's first Y byte in the source buffer
  long uv_off;         // bytes from the first Y byte to the first UV byte
  long dst_off;        // byte offset of the BGR frame in the destination buffer (ImgGeom::src_off of the same frame)
  int h, w, pitch;     // even size; bytes per row of both planes
  int aligned;         // 1: every 16-byte access of the frame's full blocks is 16-byte aligned
};
struct CscCoef { int cy, cvr, cug, cvg, cub; };   // 20-bit fixed point (include/litepi.h lp_csc)
// B frames in one launch; max_blocks = the largest (h / 2) * ceil(w / 16) of the table (2-row x 16-pixel blocks of a frame)
void launch_nv12_to_bgr(const uint8_t* src, const CscFrame* frames, uint8_t* dst, int B, int max_blocks, int matrix, hipStream_t st);
// the per-frame record of a surfaces call: SurfFrame (surface_plan.h)
// B surfaces in one launch; max_blocks as above; p010: 16-bit samples whose high byte is taken, else NV12
void launch_surfaces_to_bgr(const SurfFrame* frames, uint8_t* dst, int B, int max_blocks, bool p010, int matrix, hipStream_t st);

// ---- track_kernels.hip (sign tracking across frames, include/litepi.h lp_track_*) --------------
typedef struct lp_track TrackRec;   // (the plain name is the entry point)
struct TrackSlot {     // one slot of a stream's track table, 64 bytes, device resident between calls
  float box[4], vel[4];
  int id, hits, missed, age, det_class;
  float wsum;
  int has_vote, live;
};
struct TrackHead { int next_id, overflow, pad[2]; };   // per stream
struct TrackJob { int stream, first, nframes, pad; };  // one workgroup: frames[first .. first + nframes) of the call's frame list
#define LP_TRACK_KEY_LDS 1024   // detections of a frame whose sort key / assignment live in LDS; a larger frame uses `scratch`
struct TrackArgs {
  const lp_det* dets;       // [B * max_det]
  const int* counts;        // [B] kept counts
  TrackRec* out;            // [B * max_det]
  const TrackJob* jobs;     // [n_jobs]
  const int* frames;        // batch indices of the call's frames, grouped by job
  TrackSlot* table;         // [n_streams][T]
  TrackHead* heads;         // [n_streams]
  float* acc;               // [n_streams][T][nc] vote accumulators
  unsigned* scratch;        // [n_jobs capacity][2][max_det] when max_det > LP_TRACK_KEY_LDS, else null
  int max_det, T, nc;
  float iou_match;
  int max_age, min_hits;
  float new_conf, decay;
  int class_gate, motion;
  const lp_topk* topk;      // [B * max_det] or null: the distribution vote (lp_track_topk*) instead of (cls_class, cls_conf)
};
// topk == null runs the kernel of lp_track*, topk != null its distribution-vote instantiation
void launch_track(const TrackArgs& a, int n_jobs, hipStream_t st);
// frees every slot of `n` streams from `first` on (next_id and the overflow counter stay)
void launch_track_reset(TrackSlot* table, int T, int first, int n, hipStream_t st);

// ---- topk_kernels.hip (top-k of the classifier's distribution per detection, include/litepi.h lp_topk) ----
struct TopkArgs {
  const float* probs;       // [max_rois][nc] softmax rows as the classifier wrote them
  const int* total;         // RoiTable::total: the classified ROI count, read on the device
  const int* roi_img;       // [max_rois]
  const int* roi_slot;      // [max_rois]
  lp_topk* out;             // [B * max_det]
  int nc, k, B, max_det;
  int cap;                  // min(max_rois, B * max_det): bounds the ROI count and sizes the grid
};
// the empty record (cls = -1, prob = 0) into n_records records
void launch_topk_clear(lp_topk* out, int n_records, hipStream_t st);
// one wave per classified ROI: its top-k at (roi_img[r], roi_slot[r]); a ROI naming a record outside [B, max_det) is skipped
void launch_topk_select(const TopkArgs& a, hipStream_t st);

// ---- quality_kernels.hip (sharpness and exposure of every classified detection's crop, include/litepi.h lp_quality) ----
struct QualityArgs {
  const uint8_t* roi_rgb;   // [max_rois][S][S][3] RGB crops as roi_resize left them
  const int* total;         // RoiTable::total: the classified ROI count, read on the device
  const int* roi_img;       // [max_rois]
  const int* roi_slot;      // [max_rois]
  lp_quality* out;          // [B * max_det]
  int S, B, max_det;
  int cap;                  // min(max_rois, B * max_det): bounds the ROI count and sizes the grid
};
// the empty record (sharpness = -1, everything else 0) into n_records records
void launch_quality_clear(lp_quality* out, int n_records, hipStream_t st);
// one workgroup per classified ROI: its measure at (roi_img[r], roi_slot[r]); a ROI naming a record outside [B, max_det) is skipped
void launch_quality_measure(const QualityArgs& a, hipStream_t st);

// ---- inventory_kernels.hip (one record + best crop per finished track, include/litepi.h lp_inventory_*) ----
struct InvEntry {      // one slot of a stream's inventory, 80 bytes, device resident between calls
  lp_sign sign;        // as it would be logged (flags: LP_SIGN_HAS_CROP only)
  int open, missed, pad[2];
};
struct InvHead { int logged, pad[3]; };   // closings offered to the log since the last drain (beyond max_signs: dropped)
struct InvArgs {
  const lp_det* dets;       // [B * max_det]
  const int* counts;        // [B]
  const TrackRec* tracks;   // [B * max_det]
  const TrackJob* jobs;     // [n_jobs]; nframes == 0: flush the stream
  const int* frames;        // batch indices of the call's frames, grouped by job
  InvEntry* entries;        // [n_streams][T]
  int* frame_no;            // [n_streams]
  InvHead* head;
  lp_sign* log;             // [max_signs]
  uint8_t* log_crops;       // [max_signs][crop_bytes] or null
  uint8_t* gallery;         // [n_streams][T][crop_bytes] or null
  // crops = 1: the last pipeline call's ROI list and crops, and the record -> ROI index scatter of launch_inventory
  const uint8_t* roi_rgb;   // null: attach no crops
  const int* roi_total;
  const int* roi_img;
  const int* roi_slot;
  int* roi_of;              // [max_batch * max_det]
  int max_rois, B;
  int max_det, T, max_age, min_hits, best, max_signs, crop_bytes;
  const lp_quality* quality;   // [max_batch * max_det] or null: LP_RANK_SHARPNESS ranks a sighting by its record's sharpness instead of `best`
};
// the record -> ROI scatter (crops only), then one wave per job
void launch_inventory(const InvArgs& a, int n_jobs, hipStream_t st);
// closes every open entry of `n` streams from `first` on into the log (LP_SIGN_FLUSHED); jobs / frames / records are not read
void launch_inventory_flush(const InvArgs& a, int first, int n, hipStream_t st);

// ---- evidence_kernels.hip (a context picture of each sign's best sighting, include/litepi.h lp_evidence_*) ----
// Decide, then copy: the deciding variant of the inventory's kernel moves no pixel; it appends the work of the picture launch
// behind it to one compact list (one atomic per record).  A record can ask for two things, in this order: copy the gallery
// picture `gal` to log position copy_pos (an entry that closed with a best from an earlier call), and render window
// {x, y, w, h} of frame b into gallery picture `gal` (an entry still open whose final best lies in this call) or, with
// log_pos >= 0, into the log (an entry that took a best and closed within the call).  A best that was replaced again
// appears nowhere.  At most one record per (stream, slot) and one per record of the call.
struct EvJob { int copy_pos, b, x, y, w, h, gal, log_pos; };   // copy_pos / b / log_pos: -1 = not asked for; gal = stream * T + slot
struct EvArgs {
  const uint8_t* frames;    // the last pipeline call's BGR frames; null: crops = 0, no sighting of this call gets a picture
  const ImgGeom* fgeom;     // [B] their geometry (src_off, h, w); rows are 3 * w bytes apart
  int* win;                 // [n_streams][T][4] window of every entry's best (zeros without LP_SIGN_HAS_EVIDENCE)
  int* log_win;             // [max_signs][4]
  uint8_t* gallery;         // [n_streams][T][3 E^2]
  uint8_t* log_pics;        // [max_signs][3 E^2]
  EvJob* jobs;              // [cap_jobs]
  int* n_jobs;              // records offered to `jobs` in this call (zeroed in front of the deciding launch)
  int cap_jobs;             // n_streams * T + max_batch * max_det
  int E;
  float scale;
};
// the picture launch: `workers` x E / 8 workgroups; a worker walks the list with the workers' stride, one band of 8 picture
// rows per workgroup, and leaves at once when the list is empty.  A record's copy comes before its render, in the same
// workgroup over the same bytes: a slot closed and reused within one call ends with the old entry's picture in the log and
// the new entry's in the gallery.
void launch_evidence_pictures(const EvArgs& e, int workers, hipStream_t st);
// launch_inventory / launch_inventory_flush with the deciding kernel, then the picture launch
void launch_inventory_evidence(const InvArgs& a, const EvArgs& e, int n_jobs, hipStream_t st);
void launch_inventory_flush_evidence(const InvArgs& a, const EvArgs& e, int first, int n, hipStream_t st);

// ---- focus_kernels.hip (tracker-chosen windows + sweep, include/litepi.h lp_focus_*) ----------
struct FocusState { int cursor, unserved; };   // per stream, device resident between calls
struct FocusArgs {
  const TrackJob* jobs;     // [n_jobs] the tracker's call plan
  const int* frames;        // batch indices of the call's frames, grouped by job
  const int* fh;            // [B] frame heights, by batch index
  const int* fw;            // [B] frame widths
  const float* frf;         // [B] letterbox ratio of the whole frame (make_geom's float)
  const TrackSlot* table;   // [n_streams][T]
  FocusState* state;        // [n_streams]
  int* views;               // [B][slots][4] or null
  // the call's view tables (null for the plan alone): window slot k of frame b is ViewWin b * slots + k and view slot
  // B + b * slots + k of geom / dead; the whole-frame views are slots 0 .. B-1
  const ImgGeom* fgeom;     // [B] frame geometry (src_off)
  ViewWin* vwin;
  ImgGeom* geom;
  int* dead;                // [V] 1: the view slot is empty, its candidates do not count
  int B, T, S, motion, advance;
  int slots, side_min, side_max, border, sweep, sweep_overlap;
  float margin, small_px;
};
// one workgroup per job
void launch_focus_plan(const FocusArgs& a, int n_jobs, hipStream_t st);
// cand_count[v] = 0 for every view slot v < V with dead[v] (between the detector and the view sort)
void launch_focus_mask(const int* dead, int* cand_count, int V, hipStream_t st);

// ---- eval_kernels.hip (detections against ground truth, include/litepi.h lp_eval_*) ------------
// the evaluator's counters, device resident between calls; the num_classes ground-truth counters follow it in the same buffer
struct EvalState { long long head, dropped; int frames, pad[3]; };
// A call's plan slot: EvalFrame[max_batch], then the frames' ground-truth boxes packed in frame order.
struct EvalFrame { int first, count; };   // the frame's boxes are gts[first .. first + count)
struct EvalArgs {
  const lp_det* dets;       // [B * max_det]
  const int* counts;        // [B]
  lp_match_rec* matches;        // [B * max_det] or null
  const EvalFrame* frames;  // [B] in the plan slot
  const lp_gt* gts;         // packed, in the plan slot
  const double* thr;        // [n_thr] device copy of the configuration's thresholds
  EvalState* state;
  int* gt_per_class;        // [nc]
  lp_eval_row* log;         // [max_rows]
  int B, max_det, n_thr, max_rows, nc;
};
// one workgroup per frame, then the one-thread launch that advances head, dropped and the frame counter
void launch_eval(const EvalArgs& a, hipStream_t st);

// ---- cls_kernels.hip ------------------------------------------------------------------
// conv1 3x3/s2 (3->CO) + folded BN + ReLU on (x/255 - mean)/std of the uint8 RGB crops
void launch_cls_stem(int prec, const uint8_t* rgb, const float* w /*[27][CO]*/, const float* bias, int CO,
                     const View& out, int S, const int* m_dyn, int max_items, hipStream_t st);
// ResNet18 conv1 7x7/s2 (3 -> 64) + folded BN + ReLU on the normalised crops; w fp32 [147][64] in (ky, kx, rgb) order
void launch_cls_stem7(int prec, const uint8_t* rgb, const float* w, const float* bias, const View& out, int S, const int* m_dyn,
                      int max_items, hipStream_t st);
void launch_maxpool3x3s2(int prec, const View& in, const View& out, const int* m_dyn, int max_items, hipStream_t st);
// depthwise 3x3 pad 1 stride 1|2 + folded BN (no activation); w fp32 [9][C], bias fp32 [C]
void launch_dwconv3x3(int prec, const View& in, const View& out, const float* w, const float* bias, int stride,
                      const int* m_dyn, int max_items, hipStream_t st);
// MobileNetV2 / EfficientNet-B0 (mbnet.cpp).  act: 0 none, 1 SiLU, 2 ReLU, 3 ReLU6.
// features[0] 3x3/s2 (3 -> CO) + folded BN + activation on the normalised uint8 crops; w fp32 [27][CO] in (ky, kx, rgb) order
void launch_cls_stem_act(int prec, const uint8_t* rgb, const float* w, const float* bias, int CO, int act, const View& out, int S,
                         const int* m_dyn, int max_items, hipStream_t st);
// depthwise k x k (3 | 5), pad k/2, stride 1|2, + folded BN + activation; w fp32 [k*k][C]
void launch_dwconv_act(int prec, const View& in, const View& out, const float* w, const float* bias, int k, int stride, int act,
                       const int* m_dyn, int max_items, hipStream_t st);
// in place: scale == null: x = min(x, cap); else x[r, p, c] *= sigmoid(scale[r, c]) (squeeze-excitation gate)
void launch_mb_eltwise(int prec, const View& x, const View* scale, float cap, const int* m_dyn, int max_items, hipStream_t st);
// x.mean([2,3]) : [R,H,W,C] -> [R,1,1,C]
void launch_spatial_mean(int prec, const View& in, const View& out, const int* m_dyn, int max_items, hipStream_t st);
// softmax + argmax over fp32 logits [R,pitch]; writes probs [R,nc], ids [R], conf [R] and, when dets != null,
// scatters (id, conf) into the detection records through the ROI table
void launch_softmax_argmax(const float* logits, int pitch, int nc, float* probs, int* ids, float* conf,
                           lp_det* dets, int max_det, const RoiTable* tab, const int* m_dyn, int max_items,
                           hipStream_t st);

}  // namespace lp
