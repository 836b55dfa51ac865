/*
 * litepi.h -- C-ABI of liblitepi_hip.so: the MI355X (gfx950) implementation of
 * YOLO-LitePi's two-stage inference hot path.
 *
 * The reference (vinhisreal/YOLO-LitePi) has no FFI of its own: its seam is three
 * Python classes in src/tt100k/pipeline/e2e.py whose arithmetic runs inside NCNN /
 * ONNX Runtime / torch.  Each entry point below replaces the engine call(s) and the
 * NumPy glue cited next to it; litepi/backend.py binds them with ctypes and mirrors
 * the reference classes on top (INTEGRATION.md shows the binding).
 *
 * Conventions: every function returns 0 on success or a negative lp_status;
 * lp_last_error() returns the text of the calling thread's last failure.  Plain C
 * types only.  "host" pointers are caller-owned CPU memory, "dev" pointers are
 * device (HBM) addresses on the handle's GPU.  A handle is NOT thread-safe (the
 * reference pipeline object is not re-entrant either: e2e.py:305 creates one
 * extractor per call); use one handle per GPU.
 */
#ifndef LITEPI_H
#define LITEPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lp_handle lp_handle;

enum lp_status {
  LP_OK = 0,
  LP_ERR_ARG = -1,         /* bad argument / shape */
  LP_ERR_IO = -2,          /* cannot read model file (-> RuntimeError, e2e.py:213-216) */
  LP_ERR_GRAPH = -3,       /* graph uses something outside the YOLOv8-family op set */
  LP_ERR_HIP = -4,         /* HIP runtime failure (-> empty result, e2e.py:309-310) */
  LP_ERR_STATE = -5,       /* model not loaded / capacity exceeded */
  LP_ERR_NODEVICE = -6     /* no usable gfx950 device: the product never falls back to CPU */
};

enum lp_precision { LP_FP32 = 0, LP_FP16 = 1 };
enum lp_numerics { LP_NUMERICS_E2E = 0, LP_NUMERICS_E2E_OPTIMIZE = 1 };
enum lp_cls_arch { LP_CLS_SHUFFLENETV2 = 0, LP_CLS_RESNET18 = 1, LP_CLS_MOBILENETV2 = 2, LP_CLS_EFFICIENTNET_B0 = 3 };   /* e2e.py:320-333 */

typedef struct lp_config {
  int device;        /* HIP device ordinal */
  int precision;     /* lp_precision: storage/MFMA input type; accumulation is always fp32 */
  int max_batch;     /* images per call (capacity of every activation buffer) */
  int max_det;       /* detections kept per image after NMS; the reference keeps all (e2e.py:280-296): when more
                        survive, the max_det highest scores over all classes stay, emitted class-ascending then
                        score-descending like the reference; set it to the anchor count for keep-all semantics */
  int num_classes;   /* classifier classes (e2e.py:353 default 58) */
  int det_input;     /* detector input size (e2e.py:1040 --det_input_size, 640); with det_input_h set it is the width */
  int cls_input;     /* classifier input size (e2e.py:1041 --cls_input_size, 64) */
  int max_rois;      /* ROIs classified per call; 0 = max_batch * max_det = every kept box, as the reference
                        (e2e.py:493-497).  A smaller value that a batch exceeds makes lp_run_batch fail with
                        LP_ERR_STATE instead of leaving detections unclassified silently */
  int conv_impl;     /* 0 = MFMA kernels (product), 1 = naive direct kernels (GPU debug aid) */
  int numerics;      /* which of the reference's two pipelines the ROI stage follows:
                        0 = HybridPipeline (src/tt100k/pipeline/e2e.py:460-485, 366-370): clip x1<=w-1, x2>=x1+1 ..., PIL
                            antialiased bilinear resize;
                        1 = HybridPipelineOptimized (e2e_optimize.py:480-497, 386-390): clip to [0,w] x [0,h], drop empty
                            rectangles, cv2.resize INTER_LINEAR (no antialias).  PARITY UNPINNED (cv2 absent, no fixtures) */
  int cls_arch;      /* lp_cls_arch: classifier architecture (e2e.py:320-333 --clf_arch) */
  int det_input_h;   /* detector input height for a rectangular input (the reference's letterbox(img, (rows, columns))):
                        0 = square, det_input x det_input; otherwise a multiple of 32, at least 64 (LP_ERR_ARG).  Below,
                        SH = det_input_h ? det_input_h : det_input and SW = det_input.  The frame-view families (tiled,
                        views, focus) need SH == SW: LP_ERR_STATE otherwise.  Took reserved[0]: 0 is what every caller
                        of ABI 310 passed.  DESIGN.md 6h */
  int reserved[4];
} lp_config;

/* One detection, 32 bytes.  Mirrors one result dict of HybridPipeline.run
 * (e2e.py:519-529): bbox (float box in original-image pixels; the dict stores its
 * int truncation), det_conf, det_class, cls_class, cls_conf. */
typedef struct lp_det {
  float x1, y1, x2, y2;
  float det_conf;
  int32_t det_class;
  int32_t cls_class;   /* -1 when the ROI was not classified (e2e.py:525) */
  float cls_conf;
} lp_det;

/* Per-call stage timings in ms from HIP events on the handle's stream
 * (PipelineMetrics.t_detection / t_roi_extract / t_classification / t_total,
 * e2e.py:34-62). */
typedef struct lp_timing {
  float t_detection, t_roi_extract, t_classification, t_total;
} lp_timing;

/* ABI version of this header: bumped on every incompatible change of a signature, of lp_config's meaning or of a buffer
 * contract.  300 (round 3) vs 100: lp_run_batch takes det_conf_avg, lp_test_postprocess changed, lp_config::numerics /
 * cls_arch took two reserved words, and lp_run_batch_device's dev_counts holds 3*B int32 (was 2*B: a caller that still
 * allocates 2*B is overrun).  litepi/_ffi.py refuses a library whose lp_version() differs. */
#define LP_ABI_VERSION 310

const char* lp_last_error(void);
int lp_version(void);

/* ---- lifetime ------------------------------------------------------------------ */
void lp_default_config(lp_config* cfg);
/* replaces NCNNDetector.__init__ / PyTorchClassifier.__init__ device setup (e2e.py:198-220,353-375) */
int lp_create(const lp_config* cfg, lp_handle** out);
void lp_destroy(lp_handle* h);

/* ---- model loading ------------------------------------------------------------- */
/* replaces ncnn.Net.load_param/load_model (e2e.py:213-216): parses the NCNN text graph +
 * weight blob, checks it is a YOLOv8-family detector (Conv/Swish/C2f/SPPF/Detect+DFL),
 * BN already folded, and builds the device execution plan. */
int lp_load_detector_ncnn(lp_handle* h, const char* param_path, const char* bin_path);
/* The same from an ONNX export of the detector (what `yolo export format=onnx` writes and the reference's notebooks run through
 * ONNX Runtime; opset 11 and later, fp32 initializers, static shapes, the raw Detect output): the file is read here (protobuf
 * wire format, no dependency), lowered to the layers an NCNN export of the same model has, and planned as one: the same launches
 * and the same bits.  Both forms behave like the NCNN loader: they replace the handle's detector and drop captured graphs;
 * the model must have been exported at the handle's det_input_h x det_input.  LP_ERR_IO: the file cannot be read;
 * LP_ERR_GRAPH: a truncated or malformed file, or a node outside the lowering rules (the message names the node and its op) --
 * the handle keeps its previous detector.  The memory form reads [data, data + bytes); `name` (may be NULL) stands for the
 * model in messages.  Tensor names are the ONNX ones (the lp_debug_blob names).  DESIGN.md 6i */
int lp_load_detector_onnx(lp_handle* h, const char* onnx_path);
int lp_load_detector_onnx_memory(lp_handle* h, const void* data, size_t bytes, const char* name);
/* Pure host, no handle, no device: the lowered graph of a model file (bin_path NULL: model_path is an ONNX file; otherwise an
 * NCNN .param / .bin pair) as text, one line per layer, names left out:
 * "<type> <n_in> <n_out> <params sorted by id> <crc32 of weight> <crc32 of bias>" (a MemoryData's table stands where the weight
 * does).  *needed receives the bytes the text takes with its terminator; out may be NULL (*needed only), else cap must hold it
 * (LP_ERR_ARG). */
int lp_detector_graph_describe(const char* model_path, const char* bin_path, char* out, size_t cap, size_t* needed);
/* replaces build_classifier('shufflenetv2') + load_state_dict (e2e.py:331-340): takes the
 * torchvision shufflenet_v2_x1_0 state_dict as n named fp32 host tensors (PyTorch is used by
 * the caller only to read the .pth); BN is folded here. */
int lp_load_classifier_tensors(lp_handle* h, int n, const char* const* names,
                               const float* const* data, const int64_t* const* shapes,
                               const int* ndims);

/* ---- detector parity hook ------------------------------------------------------- */
/* replaces preprocess + ex.extract("out0") (e2e.py:222-238,305-307) for B images that are
 * already SH x SW (lp_config::det_input_h): host uint8 BGR [B,SH,SW,3] -> host fp32 out0 [B,4+nc,A]. */
int lp_detect_raw(lp_handle* h, const uint8_t* bgr, int B, float* out0);

/* ---- detector + NMS ------------------------------------------------------------- */
/* replaces NCNNDetector.detect (e2e.py:298-316: letterbox, forward, postprocess, per-class
 * NMS) for B host images of individual sizes.  dets [B*max_det] receives x1..det_class
 * (cls_* untouched); counts [B] the boxes kept per image, ordered class-ascending then
 * score-descending (e2e.py:280-296). */
int lp_detect(lp_handle* h, const uint8_t* const* imgs, const int* heights, const int* widths,
              int B, float conf, float iou, lp_det* dets, int* counts);

/* ---- full pipeline --------------------------------------------------------------- */
/* replaces HybridPipeline.run (e2e.py:443-531) for a batch: detect -> ROI clip/area filter
 * (e2e.py:465-473) -> PIL-bilinear 64x64 + normalize (e2e.py:385-389) -> ShuffleNetV2 ->
 * softmax/argmax.  dets [B*max_det]: only boxes that survive the min_area filter;
 * counts [B] their number; num_det [B] (may be NULL) the pre-filter count
 * (PipelineMetrics.num_detections, e2e.py:454); det_conf_avg [B] (may be NULL) the mean
 * detector score over the pre-filter boxes (PipelineMetrics.det_confidence_avg, e2e.py:456-457). */
int lp_run_batch(lp_handle* h, const uint8_t* const* imgs, const int* heights, const int* widths,
                 int B, float conf, float iou, int min_area,
                 lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing);

/* Same pipeline on B equally sized images already resident in HBM (dev_imgs: uint8 BGR
 * [B,H,W,3]); results stay on the device: dev_dets [B*max_det] lp_det, dev_counts [3*B] int32
 * (kept counts, then pre-filter counts, then the float bits of the mean pre-filter score).  Asynchronous on the handle's stream; this is what
 * bench.py times and what the multi-GPU gather consumes. */
int lp_run_batch_device(lp_handle* h, const void* dev_imgs, int B, int H, int W,
                        float conf, float iou, int min_area, void* dev_dets, void* dev_counts);
/* After lp_run_batch_device (synchronises the handle's stream): *kept = ROIs that survived the area filter in the last call,
 * *classified = min(kept, max_rois).  kept > classified means a user-set lp_config::max_rois was too small and
 * kept - classified detections still carry cls_class = -1 (lp_run_batch turns the same condition into LP_ERR_STATE;
 * the asynchronous device path cannot).  With max_rois = 0 (default: max_batch * max_det) it cannot happen. */
int lp_roi_overflow(lp_handle* h, int* classified, int* kept);

/* ---- multi-GPU: the one collective of the path, owned by the library (ABI 310) ------ */
/* The reference is a single process (e2e.py:1096-1134 loops over the images); sharding the images over the GPUs of a node
 * adds exactly one exchange step: every rank's fixed-capacity payload (the lp_det records + the three count words per image
 * that lp_run_batch_device wrote) goes to one root rank ("one ncclGather to rank 0", rccl.h:745).
 * RCCL is loaded lazily (dlopen of librccl.so.1 at the first of these calls): a single-GPU host without RCCL still loads
 * liblitepi_hip.so, and these four calls then fail with LP_ERR_STATE.
 *   lp_comm_unique_id : rank 0 draws the 128-byte ncclUniqueId; the launcher hands it to every rank (any out-of-band
 *                       channel: a file, an environment variable, a torch.distributed / MPI broadcast)
 *   lp_comm_init      : ncclCommInitRank on the handle's device (collective over the ranks of the communicator)
 *   lp_gather         : ncclGather of `bytes` device bytes per rank on the handle's OWN stream, i.e. ordered behind the
 *                       lp_run_batch_device that wrote them with no event; dev_recv (root only, else may be NULL) receives
 *                       world * bytes in rank order.  Asynchronous like lp_run_batch_device.
 *   lp_comm_destroy   : ncclCommDestroy (also done by lp_destroy) */
#define LP_COMM_ID_BYTES 128
int lp_comm_unique_id(void* id_out);
int lp_comm_init(lp_handle* h, const void* id, int rank, int world);
int lp_gather(lp_handle* h, const void* dev_send, size_t bytes, void* dev_recv, int root);
int lp_comm_destroy(lp_handle* h);

/* ---- tiled inference of large frames (additive to ABI 310) ------------------------- */
/* A frame larger than det_input S is also seen at native resolution: it is cut into overlapping S x S crops, every crop is
 * a view of the detector batch, and the candidates of all views of a frame go through ONE per-class greedy NMS in frame
 * coordinates (e2e.py:89-119; ties: higher (view, anchor) first).  Per axis of length L: step = S - overlap, n = 1 if
 * L <= S else 1 + ceil((L - S) / step), x_k = min(k * step, max(L - S, 0)).  A frame that needs more than one crop gets,
 * with full_frame = 1, the letterboxed whole frame as view 0 (the view lp_run_batch makes), then the crops row-major; a
 * frame that fits one tile has that single letterboxed view and gives lp_run_batch's result.  Crop pixels beyond the frame
 * edge are 114.  The frame NMS keeps two LDS flag bits per candidate slot, so one frame may span at most ~614 k slots
 * (views x anchors: 73 views of 8400 anchors); a larger frame is LP_ERR_ARG before anything is enqueued.  DESIGN.md §6b. */
typedef struct lp_tiling {
  int overlap;       /* pixels shared by neighbouring crops: 0 <= overlap < det_input */
  int full_frame;    /* 0 or 1: the letterboxed whole frame is view 0 of a frame that needs more than one crop */
  int reserved[6];   /* zero */
} lp_tiling;
/* The views of an H x W frame (pure host; no handle, no device): *n_views their number; views (may be NULL: count only)
 * receives cap x 4 ints {x, y, w, h} of each view's source window in the frame, {x0, y0, S, S} for a crop and
 * {-1, -1, W, H} for the letterboxed whole frame.  cap < *n_views with views != NULL is LP_ERR_ARG. */
int lp_tile_grid(int det_input, const lp_tiling* tiling, int H, int W, int* n_views, int* views, int cap);
/* lp_run_batch over B host frames, each seen through its views: the sum of the frames' views must not exceed max_batch
 * (LP_ERR_ARG otherwise: nothing is truncated).  dets [B*max_det], counts / num_det / det_conf_avg [B] per frame. */
int lp_run_tiled(lp_handle* h, const uint8_t* const* imgs, const int* heights, const int* widths, int B, const lp_tiling* tiling,
                 float conf, float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing);
/* lp_run_batch_device over B equally sized frames resident in HBM (uint8 BGR [B,H,W,3]): dev_dets [B*max_det],
 * dev_counts [3*B] int32 per frame (kept, pre-filter, float bits of the mean pre-filter score).  Asynchronous. */
int lp_run_tiled_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const lp_tiling* tiling,
                        float conf, float iou, int min_area, void* dev_dets, void* dev_counts);
/* The frame NMS alone (tests): n host candidates of one orig_h x orig_w frame, xyxy in frame pixels, each tagged with its
 * view (0 .. n_views-1) and anchor (0 .. 16383, unique within a view); dets / rects / count / num_det as lp_test_nms_boxes.
 * max_det <= 0: keep every survivor.  The handle's lp_set_view_merge setting applies. */
int lp_test_nms_views(lp_handle* h, const float* boxes, const float* scores, const int* classes, const int* views,
                      const int* anchors, int n, int n_views, int orig_h, int orig_w, float iou, int min_area, int max_det,
                      lp_det* dets, int* rects, int* count, int* num_det);

/* ---- frame NMS of views: match metric and box-union merge (additive to ABI 310) ---- */
/* The per-class greedy NMS above is the reference's single-image rule.  On overlapping views it leaves a sign that a view
 * border cuts as a second box inside the whole one (their IoU is small), or lets the cut box replace the whole one.  This
 * handle setting changes how the frame NMS of lp_run_tiled*, lp_run_views*, lp_run_focus* and lp_test_nms_views matches and
 * what it emits; lp_detect, lp_run_batch and lp_run_batch_device keep the reference's rule.  Everywhere these comments say
 * that one view gives lp_run_batch's result, that holds for the DEFAULT setting only: the setting applies to every frame,
 * a frame with a single view included.
 *   The candidates of a frame keep their order O: class ascending, score descending, view descending, anchor descending.
 *   thr = threshold if threshold > 0, else the call's iou.  All arithmetic is fp32, every operation rounded on its own, in
 *   the order written; keeper i, later candidate j, a = (x2 - x1) * (y2 - y1):
 *     w = max(0, min(ix2, jx2) - max(ix1, jx1));  h likewise;  inter = w * h
 *     LP_MATCH_IOU:  m = inter / (((ai + aj) - inter) + 1e-6f)
 *     LP_MATCH_IOS:  m = inter / (min(ai, aj) + 1e-6f)
 *     matched  iff  !(m <= thr)
 *   Walk O: the first candidate not yet absorbed becomes a keeper i; every later candidate j of i's class that is not yet
 *   absorbed and matches is absorbed by i.  The match always uses i's OWN box, never the growing union, so a candidate
 *   belongs to the first keeper in O that matches it.  The walk is not iterated: a ~ b, b ~ c, a !~ c gives a (with b) and c.
 *   LP_MERGE_SUPPRESS: the keeper is emitted with its own box (with LP_MATCH_IOU: the reference's rule, the default).
 *   LP_MERGE_UNION   : the emitted box is (min x1, min y1, max x2, max y2) over the keeper and everything it absorbed;
 *                      score, class and the (score, view, anchor) key stay the keeper's.
 *   The emitted boxes then go through max_det over the keepers' keys, the ROI rectangle and min_area filter, counts /
 *   num_det / the mean pre-filter score over the keepers, and the ROI list, as before.  DESIGN.md 6j. */
enum lp_match { LP_MATCH_IOU = 0, LP_MATCH_IOS = 1 };
enum lp_merge { LP_MERGE_SUPPRESS = 0, LP_MERGE_UNION = 1 };
typedef struct lp_view_merge {
  int metric;        /* lp_match */
  int mode;          /* lp_merge */
  float threshold;   /* 0 <= threshold < 1; 0 = the call's iou */
  int reserved[5];   /* zero */
} lp_view_merge;     /* 32 bytes */
/* LP_MATCH_IOU, LP_MERGE_SUPPRESS, threshold 0 */
void lp_view_merge_default(lp_view_merge* cfg);
/* pure host, no handle, no device: LP_ERR_ARG for an unknown enum value, a threshold that is NaN, negative or >= 1, a
 * non-zero reserved word or a NULL pointer */
int lp_view_merge_check(const lp_view_merge* cfg);
/* the merge of the NEXT calls of lp_run_tiled, lp_run_tiled_device, lp_run_views, lp_run_views_device, lp_run_focus,
 * lp_run_focus_device and lp_test_nms_views; NULL = the default.  Checked as by lp_view_merge_check before the handle is
 * touched.  Copied; handle state like lp_set_input_format.  A change drops nothing but makes the view families capture
 * their steps anew. */
int lp_set_view_merge(lp_handle* h, const lp_view_merge* cfg);

/* The view gather alone (tests): the views of one host H x W frame, uploaded byte_offset (0..63) bytes past an aligned
 * address, in the frame's view order -> out [n_views, S, S, 3] uint8 BGR (may be NULL: *n_views only). */
int lp_test_tile_views(lp_handle* h, const uint8_t* img, int H, int W, const lp_tiling* tiling, int byte_offset, uint8_t* out,
                       int cap, int* n_views);

/* ---- scaled views: letterbox any frame window into the detector batch (additive to ABI 310) ---- */
/* Between the one letterboxed view of lp_run_batch and the native-resolution crops of lp_run_tiled: the caller chooses the
 * scale and the place of every look at a frame.  A view is four ints {x, y, w, h}, a source window in frame pixels; x = -1
 * means the whole frame whatever its size (w, h are then ignored): the format lp_tile_grid emits.  Any other window needs
 * x, y >= 0, w, h >= 16, x + w <= W and y + h <= H for EVERY frame of the call.  One list of n_views >= 1 views applies to
 * all frames of a call.  Geometry of a window view for det_input S, in doubles, as the letterbox of an h x w image:
 *   r = min(S / h, S / w);  new_w = rint(w * r);  new_h = rint(h * r);  dw = (S - new_w) / 2;  dh = (S - new_h) / 2
 *   top = rint(dh - 0.1);  left = rint(dw - 0.1)
 *   ratio = (float)r;  pad_w = (float)(dw - r * x);  pad_h = (float)(dh - r * y)
 * (rint: round half to even); the whole-frame view is the window {0, 0, W, H}.  The view's pixels are the letterbox of
 * frame[y : y + h, x : x + w]: byte for byte what lp_test_letterbox returns for that sub-image copied out contiguously, 114
 * in the bars.  Boxes are mapped back with the three floats, in fp32 ((v - pad) / ratio), and clipped to the FRAME
 * ([0, W] x [0, H]); the candidates of all views of a frame go through the frame NMS of tiled inference in list order (ties:
 * higher (view, anchor) first); ROIs are cut from the native frame as in lp_run_tiled.  B * n_views > max_batch, or a list
 * beyond the frame NMS capacity (see tiled inference), is LP_ERR_ARG like every window error: before anything is enqueued,
 * and the handle stays usable.  DESIGN.md 6f. */
/* The window grid of an H x W frame (pure host; no handle, no device), 16 <= tile, 0 <= overlap < tile.  Per axis of length L:
 * L <= tile: one window at 0 of side L; else step = tile - overlap, n = 1 + ceil((L - tile) / step), x_k = min(k * step,
 * L - tile), side tile.  Windows come row-major; with full_frame = 1 a frame that needs more than one window gets
 * {-1, -1, W, H} first; a frame that fits one window yields only {-1, -1, W, H}.  tile = det_input on a frame with
 * H, W >= det_input reproduces lp_tile_grid.  views may be NULL (count only); cap < *n_views with views != NULL is LP_ERR_ARG. */
int lp_view_grid(int tile, int overlap, int full_frame, int H, int W, int* n_views, int* views, int cap);
/* The geometry of one view {x, y, w, h} of an H x W frame (pure host); every output may be NULL */
int lp_view_geometry(int det_input, int H, int W, const int* view, float* ratio, float* pad_w, float* pad_h,
                     int* new_w, int* new_h, int* top, int* left);
/* The letterbox of an H x W image into a det_h x det_w detector input (pure host; no handle, no device): the reference's
 * letterbox(img, new_shape = (det_h, det_w)) (e2e.py:66-86), rows x columns, in doubles:
 *   r = min(det_h / H, det_w / W);  new_w = rint(W * r);  new_h = rint(H * r);  dw = (det_w - new_w) / 2;  dh = (det_h - new_h) / 2
 *   top = rint(dh - 0.1);  left = rint(dw - 0.1)      (rint: round half to even)
 *   ratio = (float)r;  pad_w = (float)dw;  pad_h = (float)dh
 * With det_h == det_w it is the whole-frame view of lp_view_geometry, bit for bit.  It is the geometry a handle with
 * lp_config::det_input_h = det_h and det_input = det_w letterboxes with (one arithmetic).  Every output may be
 * NULL; LP_ERR_ARG for a non-positive size. */
int lp_letterbox_geometry(int det_h, int det_w, int H, int W, float* ratio, float* pad_w, float* pad_h,
                          int* new_w, int* new_h, int* top, int* left);
/* lp_run_batch over B host frames, each seen through the n_views views (views: n_views x 4 ints): dets [B*max_det],
 * counts / num_det / det_conf_avg [B] per frame.  views = {-1, ..} alone gives lp_run_batch's result. */
int lp_run_views(lp_handle* h, const uint8_t* const* imgs, const int* heights, const int* widths, int B,
                 const int* views, int n_views, float conf, float iou, int min_area,
                 lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing);
/* lp_run_batch_device over B equally sized frames resident in HBM, seen through the views; the list is a HOST array, read
 * before the call returns.  dev_dets [B*max_det], dev_counts [3*B] per frame as lp_run_tiled_device.  Asynchronous. */
int lp_run_views_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const int* views, int n_views,
                        float conf, float iou, int min_area, void* dev_dets, void* dev_counts);
/* The view gather alone (tests): the views of one host H x W frame, uploaded byte_offset (0..63) bytes past an aligned
 * address into a buffer that ends with the frame's last byte, in list order -> out [n_views, S, S, 3] uint8 BGR
 * (cap views of room; n_views <= max_batch). */
int lp_test_view_windows(lp_handle* h, const uint8_t* img, int H, int W, const int* views, int n_views,
                         int byte_offset, uint8_t* out, int cap);

/* ---- mapped views: rectify any lens into the detector batch via remap tables (additive to ABI 310) ---- */
/* A window view is an axis-aligned rectangle scaled uniformly; a mapped view takes every one of its S x S pixels from wherever
 * a per-pixel table says, and carries its boxes back to the frame through the same table.  The table is data: the caller
 * computes it once for the lens and the virtual camera wanted (a rectified pinhole looking 40 degrees right out of a fisheye
 * frame, a perspective cut of an equirectangular panorama, a rolled camera, a mirror; litepi/lens.py builds some).  Three rules,
 * one definition for host and device (csrc/view_map.h):
 * TABLE.  A map belongs to a square detector input S and a frame size H x W (1 .. 16384 a side).  xy[S][S][2] float32 holds,
 *   for view pixel (row j, column i), the frame position (x, y) it shows, in pixel-index coordinates with pixel centres at
 *   integers: cv2.remap's convention.  It is fixed once, on the host, in doubles:
 *     fx = (int32)rint(min(max((double)x, -2.0), (double)W + 1.0) * 32.0);   fy likewise with H       (rint: round half to even)
 *   i.e. fixed[S][S][2] int32 with 5 fractional bits.  A NaN anywhere is LP_ERR_ARG.
 * PIXEL.  All in int32: ix = fx >> 5 (arithmetic), ax = fx & 31, iy, ay likewise; P(r, c) = the frame's BGR pixel where
 *   0 <= r < H and 0 <= c < W, else (114, 114, 114); per channel
 *     out = (P(iy,ix)*(32-ax)*(32-ay) + P(iy,ix+1)*ax*(32-ay) + P(iy+1,ix)*(32-ax)*ay + P(iy+1,ix+1)*ax*ay + 512) >> 10
 *   This is the library's own rule, NOT cv2.remap's weight table: the same picture, not the same bytes.  No byte outside the
 *   frame's H * W * 3 is read.
 * BOX.  A candidate of a mapped view is decoded as for a crop of an S x S image (ratio 1, pads 0, clipped to [0, S]); its box
 *   (x1, y1, x2, y2) is in view coordinates.  All in fp32, every operation rounded on its own, nothing contracted:
 *     xm = (x1 + x2) * 0.5f, ym likewise; the eight sample points are the four corners and the four edge midpoints;
 *     for a point (u, v):  tu = u - 0.5f;  i = min(max((int)floorf(tu), 0), S - 2);  fu = tu - (float)i;  tv, j, fv likewise
 *       (linear extrapolation beyond the border pixels' centres);  X(r, c) = (float)fixed_x[r][c] * 0.03125f (exact);
 *       top = X(j,i) + fu * (X(j,i+1) - X(j,i));  bot = X(j+1,i) + fu * (X(j+1,i+1) - X(j+1,i));
 *       px = (top + fv * (bot - top)) + 0.5f;  py from fixed_y in the same way;
 *   the frame box is (min px, min py, max px, max py) over the eight points, clipped with fminf / fmaxf to [0, W] x [0, H].
 *   Score, class and anchor are untouched; a box that lands wholly outside becomes a zero-area box on the frame's edge and
 *   stays a candidate, as a detection in a letterbox bar does.
 * Everything behind the candidates is unchanged: the frame NMS in list order (ties: higher (view, anchor) first),
 * lp_set_view_merge, NV12 through lp_set_input_format, top-k, quality, tracker, inventory and evidence; ROIs and evidence are
 * cut from the native frame.  A handle that lists no map in a call runs exactly what it ran before.
 * Out of scope: focus slots as maps, the surfaces entry points, rectangular handles (LP_ERR_STATE), an antialiased or
 * higher-order resample (a map that shrinks the frame aliases), maps that differ per frame of one call.  DESIGN.md 6p. */
#define LP_MAP_MAX 64   /* maps of one handle; each is a device table of S * S * 8 bytes (3.3 MB at 640) */
/* The three rules, pure host (no handle, no device).  S in 2..16384; LP_ERR_ARG for NULL, a bad size or (lp_map_fixed) a NaN. */
int lp_map_fixed(const float* xy, int S, int H, int W, int32_t* fixed);                               /* xy[S][S][2] -> fixed[S][S][2] */
int lp_map_render(const int32_t* fixed, int S, const uint8_t* frame, int H, int W, uint8_t* out);  /* frame [H][W][3] -> out [S][S][3] */
int lp_map_box(const int32_t* fixed, int S, int H, int W, const float* box, float* out);             /* view box [4] -> frame box [4] */
/* A handle's maps.  lp_map_add fixes xy[S][S][2] (S = det_input) for H x W frames, keeps it as a device table and returns ids
 * 0, 1, ... in order; more than LP_MAP_MAX is LP_ERR_STATE.  lp_map_clear drops all maps (ids start at 0 again; captured
 * steps are captured anew); lp_destroy frees them.  Synchronous. */
int lp_map_add(lp_handle* h, const float* xy, int H, int W, int* id);
int lp_map_clear(lp_handle* h);
/* lp_run_views with maps: every frame is seen through the n_views listed views in list order (lp_run_views' format; views may
 * be NULL with n_views = 0) and then through the n_maps maps (ids of lp_map_add) in list order; n_views + n_maps >= 1.
 * n_maps = 0 is lp_run_views, byte for byte.  Every frame of the call must have every listed map's H x W.  A frame-size
 * mismatch, an unknown id, B * (n_views + n_maps) > max_batch or a list beyond the frame NMS capacity is LP_ERR_ARG before
 * anything is enqueued, and the handle stays usable.  A changed map list is captured anew, an unchanged one replays. */
int lp_run_mapped(lp_handle* h, const uint8_t* const* imgs, const int* heights, const int* widths, int B,
                  const int* views, int n_views, const int* maps, int n_maps, float conf, float iou, int min_area,
                  lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing);
/* lp_run_views_device with maps; both lists are HOST arrays, read before the call returns.  Asynchronous. */
int lp_run_mapped_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const int* views, int n_views,
                         const int* maps, int n_maps, float conf, float iou, int min_area, void* dev_dets, void* dev_counts);
/* The mapped gather alone (tests): one host H x W frame, uploaded as in lp_test_view_windows (the buffer ends with the
 * frame's last byte), through the n_maps maps in list order -> out [n_maps, S, S, 3] uint8 BGR (cap views of room). */
int lp_test_map_views(lp_handle* h, const uint8_t* img, int H, int W, const int* maps, int n_maps,
                      int byte_offset, uint8_t* out, int cap);
/* The candidate kernel alone (tests): n <= 16384 host view boxes [n][4] through map `map` -> frame boxes out [n][4]. */
int lp_test_map_boxes(lp_handle* h, int map, const float* boxes, int n, float* out);

/* ---- pixel format of the frames (additive to ABI 310) ------------------------------- */
/* Hardware video decoders and capture pipelines deliver NV12: a full-resolution Y plane followed by a half-resolution
 * interleaved UV plane (U first), 1.5 bytes per pixel.  With LP_PIX_NV12 set on the handle, every entry point that takes
 * FRAMES converts them on the device into a handle-owned packed BGR buffer and runs unchanged on that buffer, so the result
 * equals the result on the converted frames.  The conversion is limited-range YCbCr -> 8-bit BGR in 20-bit fixed point (the
 * arithmetic OpenCV publishes for COLOR_YUV2BGR_NV12), all in int32, >> arithmetic:
 *   u = U - 128;  v = V - 128;  y = max(Y - 16, 0) * CY;  h = 1 << 19
 *   R = clamp((y + h + CVR * v) >> 20, 0, 255)
 *   G = clamp((y + h - CVG * v - CUG * u) >> 20, 0, 255)
 *   B = clamp((y + h + CUB * u) >> 20, 0, 255)
 *   BT601 (cv2's constants): CY 1220542, CVR 1673527, CUG 409993, CVG 852492, CUB 2116026
 *   BT709 (HD video)       : CY 1220542, CVR 1880097, CUG 223347, CVG 558891, CUB 2214593
 * NV12 needs even H and W, pitch >= W, uv_offset >= pitch * H and frame_stride >= one frame; for LP_PIX_BGR8 the layout
 * fields must be 0.  Anything else, an unknown enum value or a non-zero reserved word is LP_ERR_ARG at the call that sees it
 * (lp_set_input_format for what needs no frame size, the frame-taking call for what does), before anything is enqueued.
 * lp_detect_raw, lp_classify and the lp_test_* hooks other than lp_test_convert_frames keep taking BGR.  DESIGN.md 6c. */
enum lp_pixfmt { LP_PIX_BGR8 = 0, LP_PIX_NV12 = 1 };
enum lp_csc    { LP_CSC_BT601_LIMITED = 0, LP_CSC_BT709_LIMITED = 1 };
typedef struct lp_frame_format {
  int pixfmt;            /* lp_pixfmt */
  int matrix;            /* lp_csc; ignored for BGR8 */
  int pitch;             /* bytes per row of the Y plane and of the UV plane; 0 = W (tight) */
  int reserved0;
  int64_t uv_offset;     /* bytes from a frame's first Y byte to its first UV byte; 0 = pitch * H */
  int64_t frame_stride;  /* lp_*_device only: bytes between consecutive frames; 0 = uv_offset + pitch * H / 2 */
  int reserved[6];       /* zero */
} lp_frame_format;

/* pure host, no handle, no device: validates fmt (NULL = packed BGR) for an H x W frame and resolves the zeros: *uv_offset
 * (0 for BGR8) and *frame_bytes, the bytes of one frame (H * W * 3 for BGR8); either may be NULL */
int lp_frame_layout(const lp_frame_format* fmt, int H, int W, int64_t* uv_offset, int64_t* frame_bytes);
/* the format of the frames given to the NEXT calls of lp_detect, lp_run_batch, lp_run_batch_device, lp_run_tiled,
 * lp_run_tiled_device, lp_run_views, lp_run_views_device, lp_run_focus and lp_run_focus_device; NULL = packed BGR (the default).  Copied; like lp_set_stream it is handle state.  Host frames in NV12
 * are frame_bytes each (frame_stride is ignored for them). */
int lp_set_input_format(lp_handle* h, const lp_frame_format* fmt);
/* the converter alone (tests): B host frames of one size (contiguous, frame_stride apart), uploaded byte_offset (0..63)
 * bytes past an aligned address -> out_bgr [B,H,W,3] */
int lp_test_convert_frames(lp_handle* h, const uint8_t* frames, int B, int H, int W, const lp_frame_format* fmt,
                           int byte_offset, uint8_t* out_bgr);

/* ---- decoder surfaces in place (additive to ABI 310) --------------------------------- */
/* A decoder pool hands out every frame as a surface of its own: its own device address, often a separate chroma allocation,
 * a pitch per plane, cameras of different sizes side by side, 10-bit streams as P010.  The calls below take such surfaces
 * where the decoder left them: the first launch of the step converts them into the handle-owned packed BGR frames and the
 * step runs unchanged on those, so the result is DEFINED as the result of lp_run_batch_device / lp_run_views_device on the
 * packed BGR frames the conversion gives, byte for byte; tracker, inventory and lp_set_view_merge work behind it unchanged.
 *   - `surfaces` is a HOST array of B records; it is read before the call returns.
 *   - The call is asynchronous on the handle's stream, like lp_run_batch_device: the caller keeps the surfaces' memory alive
 *     and unwritten until the stream has passed the call.
 *   - The handle's lp_set_input_format state is neither read nor changed.
 *   - The surfaces' addresses and pitches are data of the step, not part of its identity: surfaces that rotate through a
 *     pool replay one captured step, with no host synchronisation in the steady state.
 *   - lp_run_surfaces_device takes surfaces of individual sizes and runs on rectangular handles (lp_config::det_input_h);
 *     lp_run_views_surfaces_device needs every surface of one size and is LP_ERR_STATE on a rectangular handle, like its twin.
 *   - LP_SURF_NV12: 8-bit samples; exactly the formula and constants of lp_frame_format above (BT.601 / BT.709 limited range,
 *     20-bit fixed point).
 *   - LP_SURF_P010: 16-bit little-endian samples with the value in the high bits.  Only the HIGH BYTE of each sample is
 *     read: Y = s >> 8, likewise U and V, then the NV12 formula.  The low byte may hold anything, so P016 surfaces are taken
 *     the same way.  This is truncation (10 bits dropped to 8 without dither); it is this project's contract.
 *   - LP_ERR_ARG before anything is enqueued, the handle staying usable, for: a NULL fmt or surfaces; an unknown pixfmt or
 *     matrix; a non-zero reserved word; B outside 1..max_batch; a NULL plane; an odd or non-positive height or width; a
 *     negative pitch; a non-zero pitch below the row's bytes (W for NV12, 2 * W for P010, both planes); for P010 an odd plane
 *     address or an odd pitch; unequal sizes in the views variant.  Any address and any pitch are otherwise allowed.
 * DESIGN.md 6k. */
enum lp_surface_pixfmt { LP_SURF_NV12 = 1, LP_SURF_P010 = 2 };
typedef struct lp_surface {          /* 48 bytes; one decoded frame where the decoder left it */
  const void* plane[2];  /* DEVICE addresses: [0] luma rows, [1] interleaved chroma rows, U first */
  int pitch[2];          /* bytes per row of each plane; 0 = tight */
  int height, width;     /* luma size in pixels, both even */
  int reserved[4];       /* zero */
} lp_surface;
typedef struct lp_surface_format { int pixfmt; /* lp_surface_pixfmt */ int matrix; /* lp_csc */ int reserved[6]; /* zero */ } lp_surface_format;

/* pure host, no handle, no device: every rule above that needs no handle (B >= 1) */
int lp_surfaces_check(const lp_surface_format* fmt, const lp_surface* s, int B);
/* the plain pipeline (what lp_run_batch_device does) on B surfaces of individual sizes */
int lp_run_surfaces_device(lp_handle* h, const lp_surface_format* fmt, const lp_surface* surfaces, int B, float conf, float iou,
                           int min_area, void* dev_dets, void* dev_counts);
/* what lp_run_views_device does; every surface of one size */
int lp_run_views_surfaces_device(lp_handle* h, const lp_surface_format* fmt, const lp_surface* surfaces, int B, const int* views,
                                 int n_views, float conf, float iou, int min_area, void* dev_dets, void* dev_counts);
/* the converter alone (tests) on device surfaces -> the packed BGR frames, downloaded one after another (H * W * 3 bytes
 * each); its output sits between guard zones that are checked, as in lp_test_convert_frames.  Synchronous. */
int lp_test_convert_surfaces(lp_handle* h, const lp_surface_format* fmt, const lp_surface* surfaces, int B, uint8_t* out_bgr);
/* captured steps of the handle: entries in the cache, and since lp_create the calls that ran eagerly / were captured / were
 * replayed; any pointer may be NULL */
int lp_graph_stats(lp_handle* h, int* entries, int64_t* eager, int64_t* captures, int64_t* replays);

/* ---- sign tracking across frames (additive to ABI 310) ------------------------------ */
/* A tracker turns the per-frame lp_det records of a frame SEQUENCE into identities with a voted class.  It consumes the
 * records where lp_run_batch_device / lp_run_tiled_device left them, on the handle's stream, and keeps its track table in
 * HBM between calls.  n_streams independent sequences (cameras) are tracked side by side; the frames of one stream are
 * consumed in batch order.  Nothing in the reference tracks: the contract is the rule below (tests/tracking_ref.py restates
 * it in NumPy).  All arithmetic is fp32, every operation rounded on its own (nothing contracted), in the order written.
 * Per frame of a stream:
 *   1 predict  for every live track dt = missed + 1; pred = box + vel * (float)dt per coordinate (motion = 0: pred = box)
 *   2 match    the frame's detections are taken in descending det_conf (order of the fp32 bit patterns as signed
 *              magnitudes; ties: lower record index first).  Each takes the track of highest IoU with IoU > iou_match among
 *              the live tracks not yet claimed in this frame (class_gate: and of equal det_class); ties: lower slot.  With the
 *              detection as i and the predicted box as j, a = (x2 - x1) * (y2 - y1) of each:
 *                w = max(0, min(ix2, jx2) - max(ix1, jx1)); h likewise; inter = w * h
 *                iou = inter / (((ai + aj) - inter) + 1e-6f)
 *              A NaN never matches.
 *   3 update   a matched track: motion = 1: vel = (det_box - box) / (float)dt; then box = det_box; hits += 1; missed = 0;
 *              and if 0 <= cls_class < num_classes (the vote): acc[c] *= vote_decay for every class c;
 *              wsum = wsum * vote_decay + cls_conf; acc[cls_class] += cls_conf
 *   4 age      every live track not matched in this frame: missed += 1, freed when missed > max_age; every surviving track
 *              that was live before this frame: age += 1
 *   5 birth    the unmatched detections with det_conf >= new_conf, in record order, take the lowest free slot (slots freed
 *              in step 4 included): id = next_id[stream]++ (from 1), vel = 0, hits = 1, missed = 0, age = 0, acc = 0, wsum = 0,
 *              then the detection's own vote as in step 3.  With no free slot the detection stays untracked and the stream's
 *              overflow counter goes up.
 *   6 emit     one lp_track per record with its track's state after the frame: voted_class = argmax of acc (ties: lower
 *              class), voted_conf = acc[voted_class] / wsum (0 unless wsum > 0).
 * A kept count outside 0..max_det is clamped to that range.  Like every kernel of the library the tracker flushes fp32
 * denormals to zero, inputs and results: a vote that vote_decay has shrunk below 2^-126 (0.9: after ~800 matched frames
 * without a vote for that class) counts as 0.  DESIGN.md 6d. */
typedef struct lp_track_config {
  int n_streams;      /* 1..1024 independent frame sequences (cameras) */
  int max_tracks;     /* 1..256 live tracks per stream */
  float iou_match;    /* 0 <= v < 1; a detection matches a track when IoU > iou_match (default 0.3) */
  int max_age;        /* >= 0; a track unmatched for MORE than max_age consecutive frames is freed (default 5) */
  int min_hits;       /* >= 1; flag bit 0 (confirmed) once hits >= min_hits (default 3) */
  float new_conf;     /* an unmatched detection starts a track when det_conf >= new_conf (default 0) */
  float vote_decay;   /* 0 < d <= 1 (default 1) */
  int class_gate;     /* 0/1: a match needs equal det_class (default 1) */
  int motion;         /* 0 = predicted box is the last box; 1 = constant velocity (default 1) */
  int reserved[7];    /* zero */
} lp_track_config;

/* 32 bytes, parallel to lp_det: record i of frame b describes dets[b*max_det+i].  A struct tag only (write `struct lp_track`):
 * the plain name is the entry point lp_track() below, and C keeps typedef names and functions in one name space. */
struct lp_track {
  int32_t track_id;    /* >= 1; 0 = untracked (below new_conf, or the table was full) */
  int32_t slot;        /* table slot 0..max_tracks-1, -1 when untracked */
  int32_t hits;        /* frames in which the track was matched, birth included */
  int32_t age;         /* frames since birth, 0 in the birth frame */
  int32_t voted_class; /* -1 while the track has no vote */
  float   voted_conf;  /* acc[voted_class] / wsum, 0 with no vote */
  float   vote_weight; /* wsum */
  int32_t flags;       /* bit 0 confirmed, bit 1 born in this frame */
};
typedef struct lp_track lp_track_rec;   /* the record type under a plain name */
#define LP_TRACK_CONFIRMED 1
#define LP_TRACK_BORN 2

typedef struct lp_track_state {   /* 64 bytes: one live track of lp_tracker_snapshot */
  int32_t slot, track_id;
  float x1, y1, x2, y2;           /* last matched box */
  float vx1, vy1, vx2, vy2;       /* velocity per frame of each coordinate */
  int32_t hits, missed, age, det_class;
  float wsum;
  int32_t has_vote;               /* 0 until a detection with a classifier result was matched */
} lp_track_state;

void lp_track_default_config(lp_track_config* cfg);
/* pure host, no handle, no device: LP_ERR_ARG for a value outside the ranges above, a non-zero reserved word or NULL */
int lp_track_config_check(const lp_track_config* cfg);
/* one tracker per handle; calling it again replaces the tracker and restarts the ids at 1 */
int lp_tracker_create(lp_handle* h, const lp_track_config* cfg);
int lp_tracker_destroy(lp_handle* h);   /* also done by lp_destroy */
/* frees the tracks of one stream (-1: of all); next_id keeps counting, so an id is never reused during a tracker's life.
 * Asynchronous on the handle's stream. */
int lp_tracker_reset(lp_handle* h, int stream);
/* dev_dets [B*max_det] lp_det and dev_counts (kept counts = its first B words) as lp_run_batch_device / lp_run_tiled_device
 * wrote them; stream_ids: HOST array of B ints (NULL: every frame belongs to stream 0), read before the call returns;
 * dev_tracks [B*max_det] lp_track, of which only the first count[b] records of frame b are written.  Asynchronous on the
 * handle's stream, i.e. ordered behind the pipeline call with no event; any number of calls may be enqueued without a
 * synchronise in between.  LP_ERR_STATE without a tracker; LP_ERR_ARG for B outside 1..max_batch, a stream id outside
 * 0..n_streams-1 or record buffers that are not 16-byte aligned, before anything is enqueued. */
int lp_track_device(lp_handle* h, const void* dev_dets, const void* dev_counts, int B, const int* stream_ids, void* dev_tracks);
/* the same on host records as lp_run_batch / lp_run_tiled return them (uploads, runs the same kernel, downloads; synchronous) */
int lp_track(lp_handle* h, const lp_det* dets, const int* counts, int B, const int* stream_ids, struct lp_track* tracks);
/* synchronises; the live tracks of a stream in slot order, coasting ones included: *n their number, out (may be NULL: count
 * only; cap < *n is LP_ERR_ARG) their state, acc (may be NULL) the [*n, num_classes] vote accumulators, next_id / overflow
 * (may be NULL) the stream's next id and the number of detections that found the table full */
int lp_tracker_snapshot(lp_handle* h, int stream, lp_track_state* out, int cap, int* n, float* acc, int* next_id, int* overflow);

/* ---- sign inventory: one record and best crop per finished track (additive to ABI 310) ---- */
/* The tracker gives every detection an identity; the inventory turns the two record streams (lp_det, lp_track) into the
 * de-duplicated list of signs: one lp_sign per finished track, with the crop of its best sighting, logged on the device
 * when the track ends.  It sees only the records of each frame (a separate launch behind the tracker's; the tracker and its
 * outputs are unchanged) and mirrors the tracker's ageing.  It belongs to the tracker: lp_tracker_create called again and
 * lp_tracker_destroy destroy it; lp_tracker_reset leaves it alone (the orphaned entries close by the rule).
 * Per stream it holds max_tracks entries, indexed by tracker slot, and a frame counter, 0 at creation and never reset
 * (neither by lp_tracker_reset nor by lp_inventory_flush).  Per frame of a stream, with t = the counter's value:
 *   1 sight   among the frame's first count records (count clamped to 0..max_det), a record with track_id > 0 and
 *             0 <= slot < max_tracks sights its slot.  A slot out of range is ignored; if several records name one slot, the
 *             lowest record index counts (the tracker produces neither; host callers can)
 *   2 close   an open entry closes if its slot is sighted with another id, or if it is not sighted and
 *             missed + 1 > max_age (the tracker's max_age).  An open entry that is not sighted and does not close: missed += 1
 *   3 log     the closing entries with hits >= min_hits are appended to the log in ascending slot order, as one block per
 *             (stream, frame).  When the block does not fit, the lowest slots that fit are written and `dropped` grows by
 *             the rest.  Across the streams of one call the order of blocks is unspecified; within a stream it is frame order
 *   4 open /  a sighted slot with no open entry opens one: first_frame = t, and its first sighting is its best whatever its
 *     update  quality.  Every sighted entry takes last_frame = t, hits, voted_class, voted_conf and vote_weight from the
 *             lp_track record, and missed = 0.  Quality q in fp32, each operation rounded on its own:
 *               LP_BEST_AREA (x2 - x1) * (y2 - y1); LP_BEST_DET_CONF det_conf; LP_BEST_CLS_CONF cls_class >= 0 ? cls_conf : -1.0f
 *             (under LP_RANK_SHARPNESS, lp_inventory_set_rank below: q = the sharpness of the record's lp_quality instead)
 *             A later sighting replaces the best iff q > best_quality (ties keep the earlier sighting; a NaN never replaces).
 *             Replacing copies the box, det_class, best_frame = t, best_quality = q and, with crops = 1 and a crop for that
 *             record, the crop; LP_SIGN_HAS_CROP is set or cleared for that sighting
 *   5 the counter advances.
 * lp_inventory_flush closes every open entry of the stream as step 3 does, with LP_SIGN_FLUSHED (the end of a video).
 * tests/inventory_ref.py restates the rule in NumPy.  DESIGN.md 6e. */
enum lp_best { LP_BEST_AREA = 0, LP_BEST_DET_CONF = 1, LP_BEST_CLS_CONF = 2 };
typedef struct lp_inventory_config {
  int max_signs;    /* capacity of the log of finished signs, 1 .. 1<<20 (default 4096) */
  int keep_crops;   /* 0/1 (default 1): keep the classifier's input crop of every track's best sighting */
  int best;         /* one of enum lp_best; default LP_BEST_AREA */
  int min_hits;     /* >= 0; a finished track is logged only with hits >= min_hits; 0 (default) = the tracker's min_hits */
  int reserved[12]; /* zero */
} lp_inventory_config;

typedef struct lp_sign {          /* 64 bytes */
  int32_t stream, track_id;
  int32_t first_frame, last_frame;   /* frame numbers of the first and the last sighting */
  int32_t hits;                      /* lp_track::hits of the last sighting */
  int32_t voted_class; float voted_conf, vote_weight;   /* of the last sighting's lp_track record */
  int32_t best_frame; float best_quality;
  float x1, y1, x2, y2;              /* box of the best sighting */
  int32_t det_class;                 /* of the best sighting */
  int32_t flags;                     /* LP_SIGN_HAS_CROP 1, LP_SIGN_FLUSHED 2 */
} lp_sign;
#define LP_SIGN_HAS_CROP 1
#define LP_SIGN_FLUSHED 2

void lp_inventory_default_config(lp_inventory_config* cfg);
/* pure host, no handle, no device: LP_ERR_ARG for a value outside the ranges above, a non-zero reserved word or NULL */
int lp_inventory_config_check(const lp_inventory_config* cfg);
/* LP_ERR_STATE without a tracker; calling it again replaces the inventory (the log is lost, the frame counters restart).
 * Memory: the gallery of best crops is n_streams x max_tracks x 3 * cls_input^2 bytes (keep_crops only), the log
 * max_signs x (64 + 3 * cls_input^2).  keep_crops needs a cls_input that is a multiple of 4 (crops move 16 bytes per lane). */
int lp_inventory_create(lp_handle* h, const lp_inventory_config* cfg);
int lp_inventory_destroy(lp_handle* h);
/* dev_dets, dev_counts, dev_tracks, B and stream_ids exactly as the preceding lp_track_device took and wrote them.
 * Asynchronous on the handle's stream, ordered behind that call with no event; any number of calls may be enqueued without a
 * synchronise.  crops = 1 asserts that frames 0..B-1 of this call are frames 0..B-1 of the last pipeline call on this handle
 * (lp_run_batch, lp_run_batch_device, lp_run_tiled, lp_run_tiled_device, lp_run_views, lp_run_views_device, lp_run_focus,
 * lp_run_focus_device; the tiled, the views and the focus ones index frames, not views), whose ROI
 * list and classifier input crops the handle still holds: record (b, slot) has a crop iff the ROI list names it among its
 * first `total` entries.  crops = 0 attaches no crops.  LP_ERR_STATE without a tracker or an inventory; LP_ERR_ARG for B
 * outside 1..max_batch, a stream id out of range, crops outside 0/1, crops = 1 with keep_crops = 0, or record buffers that
 * are not 16-byte aligned, before anything is enqueued.  The ROI list names each record at most once (the pipeline's does;
 * a list installed with lp_test_set_rois that names one twice gets either crop). */
int lp_inventory_device(lp_handle* h, const void* dev_dets, const void* dev_counts, const void* dev_tracks, int B,
                        const int* stream_ids, int crops);
/* the same on host records (uploads [B * max_det] records of both kinds, runs the same kernel; synchronous) */
int lp_inventory(lp_handle* h, const lp_det* dets, const int* counts, const struct lp_track* tracks, int B, const int* stream_ids,
                 int crops);
/* closes every open entry of a stream (-1: of all streams) into the log, with LP_SIGN_FLUSHED; asynchronous */
int lp_inventory_flush(lp_handle* h, int stream);
/* synchronises.  *n = the logged signs, *dropped (may be NULL) = the signs lost to a full log since the last drain.
 * out == NULL: the numbers only, nothing is consumed.  cap < *n: LP_ERR_ARG, nothing is consumed.  Otherwise out receives
 * the *n signs, crops (may be NULL) their [*n, S, S, 3] uint8 RGB crops (S = cls_input: the bytes the classifier read; zeros
 * for a sign without LP_SIGN_HAS_CROP), and the log is emptied.  Only a drain resets the count of offered signs: it is an
 * int32, so drain at least once per 2^31 finished signs (a log that is never drained wraps and then reports 0 / 0). */
int lp_inventory_drain(lp_handle* h, lp_sign* out, uint8_t* crops, int cap, int* n, int* dropped);
/* synchronises; the open entries of a stream in slot order as they would be logged now (out may be NULL: *n only;
 * cap < *n is LP_ERR_ARG) */
int lp_inventory_open(lp_handle* h, int stream, lp_sign* out, int cap, int* n);
/* test hooks: put a ROI list (img[r], slot[r]) and its R crops [R, S, S, 3] into the handle as a pipeline call would leave
 * them / download the last call's (crops, img, slot may be NULL; cap < *n is LP_ERR_ARG when any is given) */
int lp_test_set_rois(lp_handle* h, const uint8_t* crops, const int* img, const int* slot, int R);
int lp_debug_rois(lp_handle* h, uint8_t* crops, int* img, int* slot, int cap, int* n);

/* ---- evidence store: a context picture of each sign's best sighting (additive to ABI 310) ---- */
/* The crop of an lp_sign is the classifier's input: the box alone, squashed to a square, RGB.  The evidence store adds what a
 * person reviewing the list needs: per open entry an E x E BGR picture of the best sighting's SURROUNDINGS, cut from the
 * native frame on the device, carried into the log when the entry closes and drained with the sign.  It belongs to the
 * inventory as the inventory belongs to the tracker: lp_inventory_create called again, lp_inventory_destroy,
 * lp_tracker_create called again and lp_tracker_destroy destroy it.  Without a store nothing changes: no existing path gains
 * a launch, a device branch or a buffer.
 * The rule extends step 4 of the inventory's rule and changes nothing else.  When a sighting becomes an entry's best (the
 * first sighting, or q > best_quality), box, best_frame and crop are replaced as above, and with a store:
 *   crops = 0 for the call: LP_SIGN_HAS_EVIDENCE is cleared for that sighting (its window is zeros)
 *   crops = 1: with the frame of that record H x W and its box {x1, y1, x2, y2}, all fp32, every operation rounded on its
 *     own, nothing contracted, fmaxf / fminf returning the non-NaN operand:
 *       bw = x2 - x1;  bh = y2 - y1
 *       has  = H >= 16 && W >= 16 && bw > 0 && bh > 0            (false for a NaN)
 *       side = (int)fminf(fmaxf(ceilf(scale * fmaxf(bw, bh)), 16.f), 16384.f)
 *       w = min(side, W);  h = min(side, H)
 *       cx = (int)fminf(fmaxf(floorf((x1 + x2) * 0.5f), 0.f), (float)W);   cy likewise with y and H
 *       x = min(max(cx - w / 2, 0), W - w);   y likewise
 *     LP_SIGN_HAS_EVIDENCE is set iff has (else the window is zeros), and the entry's picture becomes the scaled view of
 *     window {x, y, w, h} of that frame for a detector input of E: the geometry of lp_view_geometry(E, H, W, win, ...), the
 *     bytes of the window gather of lp_run_views (tests/views_ref.make_view(frame, E, win)[0]), 114 in the bars.
 *   This is the focus plan's `place` step with side_min = 16, a fixed side_max and margin = scale.  No ROI crop is needed: a
 *   record that min_area or max_rois left unclassified still gets a picture.  The resampling is plain bilinear like every
 *   view: a window many times E is aliased; an antialiased resample is out of scope.
 * "The frame" of record (b, i) is frame b of the last pipeline call on the handle: the call's BGR frames for lp_run_batch*,
 * the native frame (never a view) for the tiled, views and focus families, the converted BGR frame the handle holds for
 * NV12 and surface calls.  For the *_device entry points with BGR frames the pictures are cut from the CALLER'S buffer: it
 * must stay alive and unwritten until the stream has passed the lp_inventory* call.
 * An entry that closes is logged with its picture and window; lp_inventory_flush does the same.
 * How it runs: with a store the inventory's launch only decides and appends what is to be moved to one compact list; a
 * second plain launch behind it moves the pixels: 256 workers x E / 8 bands of 8 picture rows, each worker walking the list
 * with the workers' stride (an empty list costs the launch alone) -- first gallery -> log for entries that closed with a best from an earlier call,
 * then frame -> gallery for open entries whose final best lies in this call and frame -> log for entries that took a best
 * and closed within the call.  A best replaced again within the call is never rendered.  No host synchronisation; any
 * number of calls may be in flight.  tests/evidence_ref.py restates the rule in NumPy.  DESIGN.md 6l. */
typedef struct lp_evidence_config {   /* 32 bytes */
  int size;          /* E: side of the picture, a multiple of 16, 32..256 (default 128) */
  float scale;       /* 1 <= scale <= 16: the window's side is scale x the box's longer side (default 2) */
  int reserved[6];   /* zero */
} lp_evidence_config;
#define LP_SIGN_HAS_EVIDENCE 4

void lp_evidence_default_config(lp_evidence_config* cfg);
/* pure host: LP_ERR_ARG for a value out of range, a NaN scale, a non-zero reserved word or NULL */
int lp_evidence_config_check(const lp_evidence_config* cfg);
/* pure host: the rule's window of `box` {x1, y1, x2, y2} on an H x W frame into win {x, y, w, h} (zeros without a picture)
 * and *has; the same header function the kernel runs (csrc/evidence_window.h).  LP_ERR_ARG for a bad configuration, NULL,
 * or H, W < 1 */
int lp_evidence_window(const lp_evidence_config* cfg, int H, int W, const float* box, int* win, int* has);
/* LP_ERR_STATE without an inventory, LP_ERR_ARG when the inventory has keep_crops = 0; calling it again replaces the store
 * (open entries keep their records and lose their pictures: their flag is cleared).  Memory: a gallery of
 * n_streams x max_tracks x 3 E^2 bytes and a log of max_signs x (3 E^2 + 16) bytes, plus 48 bytes per (stream, track) and
 * 32 per (max_batch x max_det) record of work tables.  At the defaults (E = 128: 48 KB a picture; 1 stream x 64 tracks,
 * max_signs 4096) 3 MB + 192 MB; at E = 64, 0.75 MB + 48 MB; at the limits (E = 256, 192 KB a picture) a log of
 * max_signs = 1 << 20 would be 192 GB: size max_signs to the drain interval. */
int lp_evidence_create(lp_handle* h, const lp_evidence_config* cfg);
int lp_evidence_destroy(lp_handle* h);
/* lp_inventory_drain, and additionally evidence [*n, E, E, 3] uint8 BGR (the frames' byte order) and windows [*n, 4]
 * {x, y, w, h}; both zeros for a sign without LP_SIGN_HAS_EVIDENCE; either may be NULL.  LP_ERR_STATE without a store.
 * lp_inventory_drain keeps working on a handle with a store: it drains the signs and discards their pictures. */
int lp_inventory_drain_evidence(lp_handle* h, lp_sign* out, uint8_t* crops, uint8_t* evidence, int* windows, int cap, int* n,
                                int* dropped);
/* synchronises; the pictures [*n, E, E, 3] and windows [*n, 4] of a stream's open entries in slot order, parallel to
 * lp_inventory_open (either may be NULL; cap < *n is LP_ERR_ARG when any is given) */
int lp_evidence_open(lp_handle* h, int stream, uint8_t* evidence, int* windows, int cap, int* n);
/* test hook: put B host BGR frames [B, H, W, 3] of one size into the handle, with their frame geometry, as lp_run_batch
 * would leave them: lp_inventory(..., crops = 1) behind lp_test_set_rois then runs without a model.  With a store,
 * lp_inventory*(crops = 1) is LP_ERR_STATE while the handle remembers fewer than B frames; a call that reuses the handle's
 * frame buffers without being a pipeline call (lp_detect, lp_detect_raw, lp_classify) makes it forget them. */
int lp_test_set_frames(lp_handle* h, const uint8_t* frames, int B, int H, int W);

/* ---- focus views: tracker-chosen windows and a sweep in the detector batch (additive to ABI 310) ---- */
/* A focus plan connects the tracker to the scaled views: per frame the whole-frame view plus `slots` windows, chosen ON THE
 * DEVICE from the tracker's state as the last enqueued lp_track_device left it -- native-resolution windows where the small
 * tracked signs will be, the left-over slots swept over a window grid so that new signs are still picked up.  The cost per
 * frame is fixed at 1 + slots views and no call synchronises, so the captured step replays while the windows move.
 * The plan belongs to the tracker, like the inventory: lp_tracker_create called again and lp_tracker_destroy destroy it;
 * lp_tracker_reset leaves it alone.  Per stream it keeps two int32, zero at creation and never reset: a sweep `cursor` and an
 * `unserved` counter.  The frames of a call are grouped by stream exactly as lp_track_device groups them.  The j-th frame
 * (j = 0, 1, ..) of a stream within one call, of size H x W (H, W >= 16) and letterbox ratio rf (the float ratio of the
 * whole-frame view, lp_view_geometry of {-1, ..}), goes through the steps below.  All box arithmetic is fp32, every operation
 * rounded on its own, nothing contracted (tests/focus_ref.py restates the rule in NumPy):
 *   1 ask    for every live slot dt = (float)(missed + 1 + j); p = box + vel * dt per coordinate (motion = 0: p = box);
 *            x1 = max(p0, 0), y1 = max(p1, 0), x2 = min(p2, (float)W), y2 = min(p3, (float)H); bw = x2 - x1, bh = y2 - y1,
 *            m = max(bw, bh).  The track asks iff bw > 0 && bh > 0 && m * rf < small_px; a track with a NaN in p never asks.
 *            Askers are ordered by hits descending; ties: lower slot first.
 *   2 place  askers are taken in that order against the windows already placed for this frame.  An asker is covered by a
 *            placed {x, y, w, h} iff (x == 0 || x1 >= (float)(x + border)) && (x + w == W || x2 <= (float)(x + w - border))
 *            and the same two conditions in y.  A covered asker is skipped; an uncovered asker with no slot left adds 1 to
 *            `unserved`; otherwise side = clamp((int)ceilf(margin * m), side_min, side_max), w = min(side, W),
 *            h = min(side, H), cx = (int)floorf((x1 + x2) * 0.5f), x = min(max(cx - w / 2, 0), W - w), y likewise, and
 *            {x, y, w, h} is placed.
 *   3 sweep  (sweep = 1) G = the windows of lp_view_grid(side_min, sweep_overlap, 0, H, W), row-major, n = |G|.  A frame
 *            that fits one window has no sweep.  Otherwise r = min(free slots, n): the windows G[(cursor + i) % n],
 *            i = 0 .. r-1, follow the placed ones, and cursor = (cursor + r) % n.
 *   4 empty  the slots left over are empty: reported as {0, 0, 0, 0}, and they contribute no candidate to the frame NMS.
 * The views of a frame are the whole frame (view 0), then the slots in order; each window is a scaled view with the geometry
 * of lp_view_geometry, bit for bit, and everything behind the gather is tiled inference's.  DESIGN.md 6g. */
typedef struct lp_focus_config {
  int slots;          /* 1..16 window slots per frame, behind the whole-frame view */
  int side_min;       /* 16 <= side_min <= side_max; 0 = det_input */
  int side_max;       /* <= 8 * det_input (the window gather's LDS rows always fit); 0 = 2 * det_input */
  float margin;       /* >= 1: a window's side is margin x the box's longer side (default 2) */
  float small_px;     /* > 0: a track asks for a window while its longer side in the letterboxed whole frame is below this (default 32) */
  int border;         /* >= 0: a box is covered by a window only `border` pixels inside it (default 16) */
  int sweep;          /* 0/1: free slots walk the tile grid (default 1) */
  int sweep_overlap;  /* 0 <= v < side_min (default 0) */
  int reserved[8];    /* zero */
} lp_focus_config;

void lp_focus_default_config(lp_focus_config* cfg);
/* pure host, no handle, no device: LP_ERR_ARG for a value outside the ranges above (the zeros resolved with det_input), a
 * non-zero reserved word or NULL */
int lp_focus_config_check(const lp_focus_config* cfg, int det_input);
/* LP_ERR_STATE without a tracker; calling it again replaces the plan (cursor and unserved restart at zero) */
int lp_focus_create(lp_handle* h, const lp_focus_config* cfg);
int lp_focus_destroy(lp_handle* h);
/* the plan alone, synchronous: B frames of heights[b] x widths[b] (B <= max_batch), stream_ids as lp_track_device takes them;
 * views receives [B * slots * 4] host ints {x, y, w, h}; advance = 0 leaves cursor and unserved as they were */
int lp_focus_plan(lp_handle* h, int B, const int* heights, const int* widths, const int* stream_ids, int* views, int advance);
/* synchronises; the two counters of a stream (either may be NULL) */
int lp_focus_state(lp_handle* h, int stream, int* cursor, int* unserved);
/* lp_run_batch_device over B equally sized frames resident in HBM, each seen through its whole-frame view and the plan's
 * windows for its stream; dev_views (may be NULL) receives [B * slots * 4] int32, the windows used.  stream_ids is a HOST
 * array (NULL: stream 0), read before the call returns.  Asynchronous: the plan is ordered on the handle's stream behind the
 * last lp_track_device, with no synchronise.  LP_ERR_STATE without a tracker or a plan.  LP_ERR_ARG, before anything is
 * enqueued and with the handle still usable: B * (1 + slots) > max_batch, a stream id out of range, a frame below 16 pixels,
 * the frame NMS capacity exceeded (see tiled inference). */
int lp_run_focus_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const int* stream_ids,
                        float conf, float iou, int min_area, void* dev_dets, void* dev_counts, void* dev_views);
/* the same over B host frames of individual sizes, as lp_run_views; views (may be NULL) is a host array [B * slots * 4] */
int lp_run_focus(lp_handle* h, const uint8_t* const* imgs, const int* heights, const int* widths, int B, const int* stream_ids,
                 float conf, float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg,
                 lp_timing* timing, int* views);

/* ---- class distributions: top-k per detection and a distribution vote (additive to ABI 310) ---- */
/* The classifier computes a softmax over num_classes for every ROI; lp_det carries its arg-max only.  With top-k switched on,
 * every pipeline call also leaves, per detection, the k most probable classes with their probabilities in a handle-owned
 * device buffer of max_batch * max_det lp_topk records, parallel to lp_det: record i of frame b describes dets[b*max_det+i]
 * (for the tiled, views and focus families b indexes frames, not views, as the ROI list does).
 * The selection rule, for a ROI with distribution p[0..nc): p is the fp32 softmax the classifier computed, the numbers
 * lp_classify returns.  The classes are ordered by p descending, ties by class ascending.  With m = min(k, nc), entry j < m
 * holds the j-th class and its p unchanged (selection only, no arithmetic); entries j >= m hold cls = -1, prob = 0.  So
 * cls[0] == lp_det::cls_class and prob[0] has the bits of lp_det::cls_conf: the arg-max of every classifier path breaks ties
 * towards the lower class.  The comparator is one header for host and device (csrc/topk_select.h); p is expected to hold
 * no NaN.
 * A pipeline call over B frames (lp_run_batch*, lp_run_tiled*, lp_run_views*, lp_run_focus*, lp_run_surfaces_device,
 * lp_run_views_surfaces_device) writes all B * max_det records of its frames, in the same captured step, and leaves the
 * records of frames >= B alone: every ROI among the first `classified` ROIs of the ROI list (lp_roi_overflow) gets its top-k
 * at (roi_img[r], roi_slot[r]); every other record is EMPTY (all cls = -1, all prob = 0): records beyond the kept count,
 * records a user-set max_rois left unclassified, the whole call when no classifier is loaded.  The buffer holds the last
 * pipeline call's records, like the ROI list; a consumer enqueued on the handle's stream behind the call sees them, a caller
 * that wants to keep them copies them on the stream.  lp_detect, lp_detect_raw and lp_classify neither read nor write it.
 * In the host entry points the work is booked in t_classification.
 * How it runs: a plain clear launch over the B * max_det records, then the select launch: one wave per ROI, the row of
 * probabilities staged in LDS once, k rounds of a wave-wide maximum over 64-bit keys (value bits high, inverted class low),
 * each round restricted to keys below the previous winner.  The live ROI count is read on the device: no host
 * synchronisation.  While off (the default) nothing changes: the classifier gets no probability pointer, and no launch,
 * buffer or device branch is added; a handle switched on and off again runs the launches it ran before.  DESIGN.md 6m. */
#define LP_TOPK_MAX 8
typedef struct lp_topk { int32_t cls[LP_TOPK_MAX]; float prob[LP_TOPK_MAX]; } lp_topk;   /* 64 bytes, parallel to lp_det */

/* k in 1..8 switches top-k on, 0 off (the default); anything else is LP_ERR_ARG.  The buffer is allocated at the first
 * enable.  A change of k makes the run families capture their steps anew, as lp_set_view_merge does. */
int lp_topk_enable(lp_handle* h, int k);
/* the buffer's device address (stable until lp_destroy) and k; either may be NULL.  LP_ERR_STATE while off. */
int lp_topk_buffer(lp_handle* h, const void** dev_topk, int* k);
/* synchronises; the first B * max_det records.  LP_ERR_STATE while off, LP_ERR_ARG for B outside 1..max_batch. */
int lp_topk_read(lp_handle* h, lp_topk* out, int B);
/* pure host, no handle, no device: the rule above on one distribution p[0..nc).  LP_ERR_ARG for NULL, nc < 1 or k outside 1..8 */
int lp_topk_select(const float* p, int nc, int k, lp_topk* out);
/* The tracker fed the distribution: lp_track_device / lp_track with another vote, everything else (ordering, asynchrony,
 * errors) as theirs.  dev_topk is [B * max_det] lp_topk, 16-byte aligned: lp_topk_buffer's address or any device buffer; NULL
 * or a misaligned address is LP_ERR_ARG before anything is enqueued.  Steps 3 and 5 of the tracker's rule use, for a
 * detection with record t (fp32, every operation rounded on its own, nothing contracted):
 *   votes  iff  0 <= t.cls[0] < num_classes        (lp_det::cls_class / cls_conf are not read)
 *   valid j:    0 <= t.cls[j] < num_classes, j = 0..7 in order; other entries are skipped
 *   acc[c] *= vote_decay  for every class c
 *   s = 0;  for valid j in order: s = s + t.prob[j]
 *   wsum = wsum * vote_decay + s
 *   for valid j in order: acc[t.cls[j]] += t.prob[j]      (a class named twice is added twice, in j order)
 * A birth starts from acc = 0, wsum = 0 and votes the same way.  Both vote forms work on the same accumulators: a tracker may
 * be fed by either call from frame to frame, and one valid entry (cls_class, cls_conf) gives lp_track_device's result bit for
 * bit.  tests/topk_ref.py restates both rules in NumPy. */
int lp_track_topk_device(lp_handle* h, const void* dev_dets, const void* dev_counts, const void* dev_topk, int B,
                         const int* stream_ids, void* dev_tracks);
/* the same on host records (uploads, runs the same kernel, downloads; synchronous) */
int lp_track_topk(lp_handle* h, const lp_det* dets, const int* counts, const lp_topk* topk, int B, const int* stream_ids,
                  struct lp_track* tracks);
/* test hook (needs top-k on): uploads probs [R, num_classes] where the classifier leaves them, installs the ROI list
 * (img[r], slot[r]) with total = classified = R, runs clear + select for B frames and downloads B * max_det records.
 * LP_ERR_ARG for R > max_rois or an img / slot out of range. */
int lp_test_topk(lp_handle* h, const float* probs, int R, const int* img, const int* slot, int B, lp_topk* out);

/* ---- crop quality: sharpness and exposure per detection, and an inventory rank (additive to ABI 310) ---- */
/* The ROI resize leaves every ROI as an S x S x 3 uint8 RGB crop (S = cls_input): the bytes the classifier reads and the
 * inventory's gallery copies.  With quality switched on, every pipeline call also measures those crops and leaves one
 * lp_quality record per detection in a handle-owned device buffer of max_batch * max_det records, parallel to lp_det: record
 * i of frame b describes dets[b*max_det+i] (for the tiled, views and focus families b indexes frames, not views, as the ROI
 * list does).
 * The rule, for one crop c[S][S][3] in R, G, B order, integers until the last step:
 *   luma       Y(y,x) = (77*R + 150*G + 29*B + 128) >> 8, in 0..255
 *   Laplacian  on the (S-2)^2 interior pixels: L(y,x) = Y(y-1,x) + Y(y+1,x) + Y(y,x-1) + Y(y,x+1) - 4*Y(y,x), in -1020..1020
 *   sums       n = (S-2)^2, s1 = sum L, s2 = sum L^2 (int64);  N = S^2, t1 = sum Y, t2 = sum Y^2, lo = #{Y <= 4}, hi = #{Y >= 251}
 *   record     in fp64, every operation rounded on its own, each result converted to fp32:
 *                sharpness = (double)(n*s2 - s1*s1) / ((double)n*(double)n)      the variance of the Laplacian
 *                luma_mean = (double)t1 / (double)N
 *                luma_var  = (double)(N*t2 - t1*t1) / ((double)N*(double)N)
 *                clip_lo   = (double)lo / (double)N,  clip_hi = (double)hi / (double)N
 * The integer products are exact in int64 for every S <= 1024 (n*s2 and s1*s1 stay below 2^60, N*t2 and t1*t1 below 2^56).
 * Every reduction is over integers, so the result does not depend on the order of summation: the device record equals
 * lp_quality_measure of the same crop bit for bit.  The rule is one header for host and device (csrc/quality_measure.h).
 * A pipeline call over B frames (lp_run_batch*, lp_run_tiled*, lp_run_views*, lp_run_focus*, lp_run_surfaces_device,
 * lp_run_views_surfaces_device) writes all B * max_det records of its frames, in the same captured step, and leaves the
 * records of frames >= B alone: every ROI among the first `classified` ROIs of the ROI list (lp_roi_overflow) gets its
 * measure at (roi_img[r], roi_slot[r]) with LP_QUALITY_VALID; every other record is EMPTY (sharpness = -1, the other fields
 * 0, flags = 0): records beyond the kept count, records a user-set max_rois left without a crop, the whole call when no
 * classifier is loaded (no ROI list exists then).  The buffer holds the last pipeline call's records, like the ROI list.
 * lp_detect, lp_detect_raw and lp_classify neither read nor write it.  In the host entry points the work is booked in
 * t_classification.
 * How it runs: a plain clear launch over the B * max_det records, then the measure launch: one workgroup per ROI, the crop
 * read once with 16-byte loads, its luma plane held in LDS, integer reductions per wave and across waves, one thread writes
 * the record.  The live ROI count is read on the device: no host synchronisation.  While off (the default) nothing changes:
 * no launch, buffer or device branch is added; a handle switched on and off again runs the launches it ran before.
 * DESIGN.md 6o. */
typedef struct lp_quality {       /* 32 bytes, parallel to lp_det */
  float sharpness;                /* variance of the Laplacian of the crop's luma; -1 for an empty record */
  float luma_mean, luma_var;      /* 0..255, 0..16256.25 */
  float clip_lo, clip_hi;         /* share of pixels with Y <= 4 / Y >= 251 */
  int32_t flags;                  /* LP_QUALITY_VALID 1 */
  int32_t reserved[2];            /* zero */
} lp_quality;
#define LP_QUALITY_VALID 1

/* on = 1 switches quality on, 0 off (the default); anything else is LP_ERR_ARG.  The buffer is allocated at the first enable,
 * cleared to the empty record, and stable until lp_destroy.  A change makes the run families capture their steps anew; a call
 * that changes nothing does nothing.  LP_ERR_STATE when cls_input is no multiple of 4 (the crops are then not 16-byte aligned,
 * keep_crops' condition), and for on = 0 while the inventory ranks by sharpness (below). */
int lp_quality_enable(lp_handle* h, int on);
/* the buffer's device address; LP_ERR_STATE while off */
int lp_quality_buffer(lp_handle* h, const void** dev_quality);
/* synchronises; the first B * max_det records.  LP_ERR_STATE while off, LP_ERR_ARG for B outside 1..max_batch. */
int lp_quality_read(lp_handle* h, lp_quality* out, int B);
/* pure host, no handle, no device: the rule above on one crop rgb[S][S][3].  LP_ERR_ARG for NULL or S outside 3..1024. */
int lp_quality_measure(const uint8_t* rgb, int S, lp_quality* out);
/* What step 4 of the inventory's rule ranks a track's sightings by.  LP_RANK_CONFIG (the default, and what
 * lp_inventory_create restores): lp_inventory_config::best, the rule as stated there.  LP_RANK_SHARPNESS: q is the sharpness
 * field of record (b, idx) of the handle's quality buffer, read as is when the inventory call runs; an empty record gives
 * q = -1, so a sighting without a crop never replaces a measured one, and the first sighting is still the best whatever its
 * q.  Everything else in the rule is unchanged; lp_sign::best_quality carries the sharpness, and the evidence store follows
 * the same choice.  The largest sighting of a sign on a moving camera is usually the last before it leaves the frame and the
 * most blurred; this rank keeps the sharpest crop instead.
 * LP_ERR_STATE without an inventory, or for LP_RANK_SHARPNESS with quality off; LP_ERR_ARG for an unknown rank.  While the rank
 * is LP_RANK_SHARPNESS, lp_inventory_device / lp_inventory with crops = 0 are LP_ERR_ARG before anything is enqueued (the buffer
 * describes the last pipeline call, which is what crops = 1 asserts), and lp_quality_enable(h, 0) is LP_ERR_STATE. */
enum lp_rank { LP_RANK_CONFIG = 0, LP_RANK_SHARPNESS = 1 };
int lp_inventory_set_rank(lp_handle* h, int rank);
/* test hook (needs quality on): on the ROI list and crops lp_test_set_rois installed, runs clear + measure for B frames and
 * downloads B * max_det records.  LP_ERR_ARG for B outside 1..max_batch. */
int lp_test_quality(lp_handle* h, int B, lp_quality* out);

/* ---- device-side evaluation: detections against ground truth (additive to ABI 310) -- */
/* An evaluator belongs to a handle, like the tracker: a null pointer nobody else looks at until lp_eval_create.  It matches
 * the lp_det records of a call against ground-truth boxes on the device and appends one compact row per record to a log in
 * HBM; precision, recall, F1, mAP50 and mAP50-95 are then one host function over the drained rows
 * (litepi.e2e.metrics_from_rows, the tail of evaluate_predictions).  Plain launches on the handle's stream, outside the
 * captured step.  Without an evaluator nothing changes: no existing path gains a launch, a branch or a buffer.
 *
 * The rule, per frame with P records (the kept count clamped to 0..max_det) and G ground-truth boxes (0 <= G <= max_gt); the
 * host (lp_eval_match) and the device run the same header, csrc/eval_match.h:
 *   1 boxes    a record's box is its four fp32 coordinates truncated toward zero to int32 (the result dict's bbox; a NaN
 *              gives 0).  Record and ground-truth coordinates are clamped to -2^29 .. 2^29, far beyond any frame, so that
 *              nothing below leaves int64.
 *   2 IoU      of the pair (p, g), in int64: iw = max(0, min(px2, gx2) - max(px1, gx1)), ih likewise, inter = iw * ih,
 *              area = (x2 - x1) * (y2 - y1) of either box; then iou = (double)inter / ((double)(area_p + area_g - inter) + 1e-7):
 *              one fp64 add and one correctly rounded fp64 division.
 *   3 best     best(p) = the g with the largest iou(p, g), on an exact tie the HIGHER g; b(p) = that IoU.  With G == 0 or
 *              b(p) == 0 the record has no best ground truth.
 *   4 correct  per threshold thr[j] (n_thr doubles in any order): a record is a candidate if it has a best ground truth and
 *              b(p) >= thr[j]; winner(g, j) = the LOWEST record index among the candidates with best(p) == g; bit j of
 *              correct(p) is set iff p == winner(best(p), j) and the record's cls_class equals gt[best(p)].cls.  A winner of
 *              the wrong class blocks its ground truth.
 *   5 outputs  optionally one lp_match_rec per record (only the first P of a frame are written; gt = -1 and iou = 0 without a
 *              best ground truth), and always one lp_eval_row per record in the evaluator's log.  frame is the evaluator's
 *              own frame counter (it counts every frame of every call and is reset only by lp_eval_reset).  Rows are in
 *              frame order, then record order, across calls: a row's position is the log head at the start of the call plus
 *              the kept counts of the call's earlier frames plus the record index.  Rows at positions >= max_rows are not
 *              written and are counted in `dropped`; the head keeps counting.  Also kept: the number of ground-truth boxes
 *              per class (num_classes int32 counters) and the number of frames seen.
 * Against evaluate_predictions (e2e.py:656-824 of the reference): its argsort()[::-1] is an unstable sort, so its choice
 * among equal IoUs is undefined.  The `correct` matrix above equals the port's on every frame in which no record has two
 * ground-truth boxes sharing its maximal IoU at or above the lowest threshold; on the other frames the rule above holds. */
typedef struct lp_gt {   /* 32 bytes: parse_yolo_label's tuple */
  int32_t cls, x1, y1, x2, y2;
  int32_t reserved[3];
} lp_gt;
typedef struct lp_match_rec {   /* 16 bytes, one per lp_det record; the tag lp_match is the view-merge metric's enum */
  uint32_t correct;   /* bit j: correct at thr[j] */
  int32_t gt;         /* best(p), or -1 */
  double iou;         /* b(p), or 0 */
} lp_match_rec;
typedef struct lp_eval_row {   /* 16 bytes */
  float conf;         /* det_conf */
  int32_t cls;        /* cls_class */
  uint32_t correct;
  int32_t frame;
} lp_eval_row;
#define LP_EVAL_MAX_GT 256
#define LP_EVAL_MAX_THR 16
typedef struct lp_eval_config {
  int max_gt;         /* ground-truth boxes per frame, 1..256; default 64 */
  int max_rows;       /* capacity of the row log, >= 1; default 1 << 20 */
  int n_thr;          /* 1..16; default 10 */
  int reserved0;
  double thr[16];     /* default 0.5 + j * ((0.5 + 0.05) - 0.5) in double: np.arange(0.5, 1.0, 0.05)'s bit patterns */
  int reserved[8];
} lp_eval_config;
void lp_eval_default_config(lp_eval_config* cfg);
/* pure host, no handle, no device: LP_ERR_ARG for a value out of range, a NaN threshold, a non-zero reserved word or NULL */
int lp_eval_config_check(const lp_eval_config* cfg);
/* one evaluator per handle; calling it again replaces the evaluator (the log is lost, every counter restarts) */
int lp_eval_create(lp_handle* h, const lp_eval_config* cfg);
int lp_eval_destroy(lp_handle* h);   /* also done by lp_destroy */
/* asynchronous on the handle's stream: head, dropped, the frame counter and the class counts become zero */
int lp_eval_reset(lp_handle* h);
/* dev_dets [B*max_det] lp_det and dev_counts [B] as lp_run_batch_device / lp_run_tiled_device / lp_run_views_device left them;
 * gts HOST [B*max_gt] (frame b's boxes at gts[b*max_gt ..]), gt_counts HOST [B]; dev_matches [B*max_det] lp_match_rec or NULL.
 * The host arrays are read before the call returns and travel through the evaluator's ring of pinned slots, so a pageable
 * source never synchronises the stream and any number of calls may be enqueued without a synchronise in between.
 * LP_ERR_STATE without an evaluator.  LP_ERR_ARG before anything is enqueued, the handle staying usable, for B outside
 * 1..max_batch, a gt_counts[b] outside 0..max_gt, a ground-truth class outside 0..num_classes-1, NULL, or a record buffer
 * that is not 16-byte aligned. */
int lp_eval_device(lp_handle* h, const void* dev_dets, const void* dev_counts, int B, const lp_gt* gts, const int* gt_counts,
                   void* dev_matches);
/* the same on host records: upload, the same kernel, download of every frame's first P matches (matches may be NULL); synchronous */
int lp_eval(lp_handle* h, const lp_det* dets, const int* counts, int B, const lp_gt* gts, const int* gt_counts, lp_match_rec* matches);
/* synchronises.  *n = the rows in the log (at most max_rows); rows == NULL: the numbers only; cap < *n with rows != NULL is
 * LP_ERR_ARG.  gt_per_class [num_classes], frames, dropped: any may be NULL.  Nothing is reset. */
int lp_eval_drain(lp_handle* h, lp_eval_row* rows, int cap, int* n, int* gt_per_class, int* frames, int* dropped);
/* pure host, no handle, no device: the rule on one frame.  LP_ERR_ARG for NULL where a count is positive, P < 0, G < 0 or
 * n_thr outside 1..16. */
int lp_eval_match(const lp_det* dets, int P, const lp_gt* gts, int G, const double* thr, int n_thr, lp_match_rec* out);

/* ---- classifier alone ------------------------------------------------------------ */
/* replaces PyTorchClassifier.predict_batch (e2e.py:378-396) for R host BGR crops of
 * individual sizes: ids [R], probs [R*num_classes] (softmax). */
int lp_classify(lp_handle* h, const uint8_t* const* rois, const int* heights, const int* widths,
                int R, int* ids, float* probs);

/* ---- streams / profiling --------------------------------------------------------- */
int lp_set_stream(lp_handle* h, void* hip_stream);   /* NULL = the handle's own stream */
int lp_synchronize(lp_handle* h);
/* Per-launch device timing of the NEXT pipeline call (hipEvents around every kernel on the
 * launch stream).  After that call returns, lp_profile_read gives up to cap entries. */
typedef struct lp_kernel_time {
  char name[48];     /* kernel family, e.g. "conv3x3_mfma_f16" */
  char layer[32];    /* graph layer, e.g. "conv_48" */
  float ms;
  double flops;      /* algorithmic FLOPs of this launch (2*MAC), 0 for byte movers */
  double bytes;      /* algorithmic HBM bytes of this launch (inputs read once + outputs written once) */
} lp_kernel_time;
int lp_profile_next(lp_handle* h, int enable);
int lp_profile_read(lp_handle* h, lp_kernel_time* out, int cap, int* n);

/* ---- introspection (tests) -------------------------------------------------------- */
int lp_detector_info(lp_handle* h, int* num_anchors, int* num_det_classes, int* reg_max,
                     double* conv_macs_per_image);
/* Copy an intermediate detector blob of the last lp_detect_raw call to host as fp32
 * logical [B,C,H,W] (NCNN blob names, e.g. "44" = P3), B = the whole images that cap floats
 * hold: at least one; more than the handle's capacity is an error.  out NULL: only C, H, W.  Test/bisect aid. */
int lp_debug_blob(lp_handle* h, const char* blob, float* out, int64_t cap, int* C, int* H, int* W);
/* Run one convolution through the chosen kernel family on host data (tests):
 * x fp32 [N,Cin,H,W], w fp32 [Cout,Cin,k,k], bias [Cout] or NULL, res [N,Cout,Ho,Wo] or NULL. */
int lp_test_conv(lp_handle* h, int impl, const float* x, int N, int Cin, int H, int W,
                 const float* w, const float* bias, int Cout, int k, int stride, int act,
                 const float* res, float* y);
/* Decode+NMS(+ROI filter) on a host out0 tensor (tests of the post-processing kernels in isolation):
 * out0 fp32 [4+nc, A], geometry of the original image -> dets/count as lp_detect.  min_area < 0: no ROI
 * filter; >= 0: the ROI clip + area filter of e2e.py:465-473, rects [count*4] (may be NULL) receives the int
 * crop rectangles and num_det (may be NULL) the pre-filter count.  max_det <= 0: keep every survivor. */
int lp_test_postprocess(lp_handle* h, const float* out0, int nc, int A, int orig_h, int orig_w,
                        float ratio, float pad_w, float pad_h, float conf, float iou, int min_area, int max_det,
                        lp_det* dets, int* rects, int* count, int* num_det);
/* NMS + ROI clip/area filter on host boxes (xyxy, original-image pixels) given directly, bypassing the decode filter:
 * replays the reference's HybridPipeline.run ROI fixtures (e2e.py:460-485) through the device kernel. */
int lp_test_nms_boxes(lp_handle* h, const float* boxes, const float* scores, const int* classes, int n,
                      int orig_h, int orig_w, float iou, int min_area, int max_det,
                      lp_det* dets, int* rects, int* count, int* num_det);
/* PIL-exact ROI resize alone: host BGR crops -> uint8 RGB [R,S,S,3]. */
int lp_test_roi_resize(lp_handle* h, const uint8_t* const* rois, const int* heights,
                       const int* widths, int R, uint8_t* out_rgb);
/* The same kernel on R rectangles {x1, y1, x2, y2} (0 <= x1 < x2 <= W, 0 <= y1 < y2 <= H) of one host BGR frame, uploaded
 * into a buffer of exactly H*W*3 bytes: ROIs at any x offset and row alignment, and at the buffer's two ends
 * -> uint8 RGB [R,S,S,3].  (additive to ABI 310) */
int lp_test_roi_resize_rects(lp_handle* h, const uint8_t* frame, int H, int W, const int* rects, int R,
                             uint8_t* out_rgb);
/* cv2-style letterbox alone: host BGR image -> uint8 BGR [SH,SW,3] + ratio/pad (lp_config::det_input_h). */
int lp_test_letterbox(lp_handle* h, const uint8_t* img, int H, int W, uint8_t* out,
                      float* ratio, float* pad_w, float* pad_h);
/* the same with the kernel named: 0 = the launcher's choice (the tiled kernel where its LDS rows fit, else the per-pixel
 * kernel), 1 = the per-pixel kernel.  Both give the same bytes.  (additive to ABI 310) */
int lp_test_letterbox_kernel(lp_handle* h, const uint8_t* img, int H, int W, int kernel, uint8_t* out,
                             float* ratio, float* pad_w, float* pad_h);

#ifdef __cplusplus
}
#endif
#endif /* LITEPI_H */
