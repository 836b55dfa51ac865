"""The evaluator's matching rule (include/litepi.h, lp_eval_*) restated in NumPy, and the seeded scenes its tests share.

Per frame: int64 boxes (a record's fp32 coordinates truncated toward zero), float64 IoU exactly as litepi.e2e._pairwise_iou
computes it, the best ground truth of a record with the HIGHER index winning an exact tie, and per threshold the LOWEST
record index among the candidates of a ground truth as its winner; a winner of the wrong class blocks its ground truth.
"""
import numpy as np

from litepi._ffi import DET_DTYPE, EVAL_ROW_DTYPE, GT_DTYPE, MATCH_DTYPE

THR10 = np.arange(0.5, 1.0, 0.05)
COORD_MAX = 2 ** 29


def det_boxes(dets) -> np.ndarray:
    """[P, 4] int64: truncation toward zero (numpy's astype(int)), a NaN gives 0, clamped to +-2^29"""
    f = np.stack([dets["x1"], dets["y1"], dets["x2"], dets["y2"]], 1).astype(np.float64)
    f = np.where(np.isnan(f), 0.0, np.clip(f, -COORD_MAX, COORD_MAX))
    return np.trunc(f).astype(np.int64)


def gt_array(gts) -> np.ndarray:
    """[G, 5] int64 (cls, x1, y1, x2, y2) from tuples or GT_DTYPE records"""
    if isinstance(gts, np.ndarray) and gts.dtype.names:
        return np.stack([gts[k].astype(np.int64) for k in ("cls", "x1", "y1", "x2", "y2")], 1).reshape(-1, 5)
    return np.asarray(gts, dtype=np.int64).reshape(-1, 5)


def pairwise_iou(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = np.maximum(a[:, None, :2], b[:, :2])
    rb = np.minimum(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt).clip(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area_a[:, None] + area_b - inter + 1e-7)


def _best(dets, g):
    """(best [P] or -1, b [P]) of step 3, and the IoU matrix"""
    P = len(dets)
    best, b = np.full(P, -1, np.int64), np.zeros(P)
    if P == 0 or len(g) == 0:
        return best, b, np.zeros((P, len(g)))
    box = np.clip(g[:, 1:], -COORD_MAX, COORD_MAX)
    iou = pairwise_iou(det_boxes(dets), box)
    for p in range(P):
        m = iou[p].max()
        if m != 0:
            best[p], b[p] = np.flatnonzero(iou[p] == m)[-1], m
    return best, b, iou


def match(dets, gts, thr=THR10) -> np.ndarray:
    """the rule on one frame: DET_DTYPE records and ground truth -> MATCH_DTYPE records"""
    dets = np.asarray(dets, dtype=DET_DTYPE).reshape(-1)
    g = gt_array(gts)
    out = np.zeros(len(dets), dtype=MATCH_DTYPE)
    best, b, _ = _best(dets, g)
    out["gt"], out["iou"] = best, b
    for j, t in enumerate(np.asarray(thr, dtype=np.float64)):
        winner = {}
        for p in range(len(dets)):
            if best[p] >= 0 and b[p] >= t and best[p] not in winner:
                winner[int(best[p])] = p
        for gi, p in winner.items():
            if dets["cls_class"][p] == g[gi, 0]:
                out["correct"][p] |= np.uint32(1 << j)
    return out


def ties(dets, gts, thr=THR10) -> int:
    """records of the frame with two ground-truth boxes sharing their maximal IoU at or above the lowest threshold: the
    frames on which evaluate_predictions' unstable sort leaves the port's choice undefined"""
    dets = np.asarray(dets, dtype=DET_DTYPE).reshape(-1)
    g = gt_array(gts)
    if len(dets) == 0 or len(g) == 0:
        return 0
    iou = pairwise_iou(det_boxes(dets), np.clip(g[:, 1:], -COORD_MAX, COORD_MAX))
    m = iou.max(1)
    return int(((iou == m[:, None]).sum(1) > 1)[m >= np.min(thr)].sum())


def rows_of(frames, thr=THR10, first_frame: int = 0, max_det=None):
    """the log a sequence of frames [(dets, gts), ...] leaves: (EVAL_ROW_DTYPE rows, [per frame MATCH_DTYPE])"""
    rows, matches = [], []
    for k, (dets, gts) in enumerate(frames):
        dets = np.asarray(dets, dtype=DET_DTYPE).reshape(-1)[:max_det]
        m = match(dets, gts, thr)
        r = np.zeros(len(dets), dtype=EVAL_ROW_DTYPE)
        r["conf"], r["cls"], r["correct"], r["frame"] = dets["det_conf"], dets["cls_class"], m["correct"], first_frame + k
        rows.append(r)
        matches.append(m)
    return (np.concatenate(rows) if rows else np.zeros(0, dtype=EVAL_ROW_DTYPE)), matches


def gt_per_class(frames, num_classes: int) -> np.ndarray:
    out = np.zeros(num_classes, np.int32)
    for _, gts in frames:
        for c in gt_array(gts)[:, 0]:
            out[c] += 1
    return out


def result_dicts(dets):
    """the fields of HybridPipeline's result dicts that evaluate_predictions reads"""
    dets = np.asarray(dets, dtype=DET_DTYPE).reshape(-1)
    boxes = np.stack([dets["x1"], dets["y1"], dets["x2"], dets["y2"]], 1).astype(int).tolist() if len(dets) else []
    return [{"bbox": tuple(bb), "conf": float(c), "cls_class": int(k)} for bb, c, k in zip(boxes, dets["det_conf"].astype(np.float64), dets["cls_class"])]


def port_correct(dets, gts, thr=THR10) -> np.ndarray:
    """the `correct` matrix evaluate_predictions' loop builds for one frame (litepi.e2e, the reference's e2e.py:656-824)"""
    preds = result_dicts(dets)
    correct = np.zeros((len(preds), len(thr)), bool)
    if not preds or not len(gts):
        return correct
    pb = np.array([p["bbox"] for p in preds])
    pcls = np.array([p["cls_class"] for p in preds])
    g = np.array([tuple(int(v) for v in r) for r in gt_array(gts)])
    tcls, tb = g[:, 0], g[:, 1:]
    iou = pairwise_iou(pb, tb)
    for j, t in enumerate(thr):
        pi, gi = np.where(iou >= t)
        if not len(pi):
            continue
        m = np.concatenate((np.stack((pi, gi), 1), iou[pi, gi][:, None]), 1)
        if len(pi) > 1:
            m = m[m[:, 2].argsort()[::-1]]
            m = m[np.unique(m[:, 0], return_index=True)[1]]
            m = m[np.unique(m[:, 1], return_index=True)[1]]
        for p_i, g_i, _ in m:
            if pcls[int(p_i)] == tcls[int(g_i)]:
                correct[int(p_i), j] = True
    return correct


def correct_matrix(m, n_thr: int) -> np.ndarray:
    return ((m["correct"][:, None] >> np.arange(n_thr, dtype=np.uint32)[None, :]) & 1).astype(bool)


# ---- seeded scenes -------------------------------------------------------------------------------------------------------
def make_dets(boxes, conf, cls) -> np.ndarray:
    boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    d = np.zeros(len(boxes), dtype=DET_DTYPE)
    d["x1"], d["y1"], d["x2"], d["y2"] = boxes.T
    d["det_conf"], d["cls_class"], d["det_class"] = conf, cls, 0
    d["cls_conf"] = 0.5
    return d


def scene(rng, P: int, G: int, nc: int, W: int = 2048):
    """P records jittered around G ground-truth boxes on a W x W frame (30 % of them far off, 20 % with another class), with
    fractional coordinates and distinct confidences -> (DET_DTYPE records, [(cls, x1, y1, x2, y2), ...])"""
    if G == 0:
        xy = rng.integers(0, W - 100, (P, 2))
        boxes = np.concatenate([xy, xy + rng.integers(5, 90, (P, 2))], 1) + rng.random((P, 4))
        return make_dets(boxes, rng.permutation(P).astype(np.float32) / max(P, 1) * 0.9 + 0.05, rng.integers(0, nc, P)), []
    gx, gy = rng.integers(0, W - 200, G), rng.integers(0, W - 200, G)
    gw, gh = rng.integers(8, 120, G), rng.integers(8, 120, G)
    g = np.stack([rng.integers(0, nc, G), gx, gy, gx + gw, gy + gh], 1)
    src = rng.integers(0, G, P)
    sc = np.maximum(2, gw[src] // 6)
    j = lambda: rng.integers(-sc, sc + 1)  # noqa: E731
    boxes = np.stack([gx[src] + j(), gy[src] + j(), gx[src] + gw[src] + j(), gy[src] + gh[src] + j()], 1).astype(np.float64)
    far = rng.random(P) < 0.3
    boxes[far, :2] = rng.integers(0, W - 100, (int(far.sum()), 2))
    boxes[far, 2:] = boxes[far, :2] + rng.integers(5, 90, (int(far.sum()), 2))
    boxes += rng.random((P, 4)) * 0.98
    cls = np.where(rng.random(P) < 0.8, g[src, 0], rng.integers(0, nc, P))
    conf = rng.permutation(P).astype(np.float32) / max(P, 1) * 0.9 + 0.05
    return make_dets(boxes, conf, cls), [tuple(int(v) for v in r) for r in g]


def hand_frames():
    """name -> (dets, gts, thr, expected {record: (correct bits, gt)}) : the frames that pin one clause of the rule each"""
    T = THR10
    f = {}
    # two ground-truth boxes with the same IoU to the record: the higher index wins, and its class decides
    f["gt_tie_higher_g"] = (make_dets([[0, 0, 10, 10]], [0.9], [1]), [(0, 0, 0, 10, 8), (1, 0, 2, 10, 10)], T, {0: (0b0000000111111, 1)})
    # two records on one ground truth: the lower index wins at every threshold both pass
    f["two_records_lower_p"] = (make_dets([[0, 0, 10, 9], [0, 0, 10, 10]], [0.2, 0.9], [3, 3]), [(3, 0, 0, 10, 10)], T,
                                {0: (0b0011111111, 0), 1: (0b1100000000, 0)})   # IoU 0.9 / (1 + 1e-9) < 0.9 and 1 / (1 + 1e-9) >= 0.95
    # a winner of the wrong class blocks the right-class runner-up
    f["wrong_class_blocks"] = (make_dets([[0, 0, 10, 10], [0, 0, 10, 10]], [0.9, 0.8], [2, 3]), [(3, 0, 0, 10, 10)], T, {0: (0, 0), 1: (0, 0)})
    f["unclassified"] = (make_dets([[0, 0, 10, 10]], [0.9], [-1]), [(0, 0, 0, 10, 10)], T, {0: (0, 0)})
    f["zero_area"] = (make_dets([[5, 5, 5, 9], [0, 0, 10, 10]], [0.9, 0.8], [0, 0]), [(0, 0, 0, 10, 10), (0, 20, 20, 20, 20)], T,
                      {0: (0, -1), 1: (0b1111111111, 0)})
    # 12.99 -> 12 and -0.9 -> 0: the truncated box is exactly the ground truth
    f["truncation"] = (make_dets([[-0.9, 2.99, 12.99, 14.5]], [0.9], [0]), [(0, 0, 2, 12, 14)], T, {0: (0b1111111111, 0)})
    # inter 50, union 100: 50 / (100 + 1e-7) < 0.5, no candidate at 0.5; 0.45 in an unsorted list is passed
    f["on_threshold"] = (make_dets([[0, 0, 10, 5]], [0.9], [0]), [(0, 0, 0, 10, 10)], np.array([0.5, 0.45, 0.55]), {0: (0b010, 0)})
    return f
