"""NumPy statement of the frame NMS of views with a match metric and a merge mode (test infrastructure only;
include/litepi.h "frame NMS of views" states the rule).

The candidates of one frame come view-major (views ascending, anchors ascending within a view), as ``tiling_ref.merge`` takes
them.  Their order O is class ascending, score descending, view descending, anchor descending.  Walk O: the first candidate
not yet absorbed becomes a keeper; every later candidate of its class that is not yet absorbed and matches the keeper's OWN
box is absorbed by it.  All arithmetic is fp32, every operation rounded on its own.
"""
from typing import Optional, Tuple

import numpy as np

IOU, IOS = 0, 1
SUPPRESS, UNION = 0, 1

_EPS = np.float32(1e-6)


def order(scores, classes, views, anchors) -> np.ndarray:
    """O: class ascending, score descending, view descending, anchor descending"""
    s = np.asarray(scores, np.float32)
    return np.lexsort((-np.asarray(anchors, np.int64), -np.asarray(views, np.int64), -s.astype(np.float64), np.asarray(classes, np.int64)))


def match_value(bi: np.ndarray, bj: np.ndarray, metric: int) -> np.ndarray:
    """m of keeper box bi [4] against boxes bj [n, 4], fp32"""
    bi, bj = np.asarray(bi, np.float32), np.asarray(bj, np.float32).reshape(-1, 4)
    ai = (bi[2] - bi[0]) * (bi[3] - bi[1])
    aj = (bj[:, 2] - bj[:, 0]) * (bj[:, 3] - bj[:, 1])
    zero = np.float32(0)
    w = np.maximum(zero, np.minimum(bi[2], bj[:, 2]) - np.maximum(bi[0], bj[:, 0]))
    h = np.maximum(zero, np.minimum(bi[3], bj[:, 3]) - np.maximum(bi[1], bj[:, 1]))
    inter = w * h
    if metric == IOU:
        den = ((ai + aj) - inter) + _EPS
    elif metric == IOS:
        den = np.minimum(ai, aj) + _EPS
    else:
        raise ValueError(f"unknown metric {metric}")
    assert inter.dtype == np.float32 and den.dtype == np.float32
    return inter / den


def merge(boxes, scores, classes, views, anchors, iou: float, max_det: Optional[int] = None, metric: int = IOU, mode: int = SUPPRESS,
          threshold: float = 0.0, owners: bool = False) -> Tuple[np.ndarray, ...]:
    """(indices of the keepers in output order, their emitted boxes float32 [k, 4]); with max_det, the max_det best
    (score, view, anchor) keepers over all classes stay.  owners: also the keeper every candidate went to (itself for a keeper),
    before max_det."""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores, classes = np.asarray(scores, np.float32), np.asarray(classes)
    views, anchors = np.asarray(views, np.int64), np.asarray(anchors, np.int64)
    if mode not in (SUPPRESS, UNION):
        raise ValueError(f"unknown mode {mode}")
    assert np.array_equal(np.lexsort((anchors, views)), np.arange(len(scores))), "candidates must come view-major, anchors ascending"
    thr = np.float32(threshold if threshold > 0 else iou)
    O = order(scores, classes, views, anchors)
    ob, oc = boxes[O], classes[O]
    absorbed = np.zeros(len(O), bool)
    owner = np.arange(len(O), dtype=np.int64)
    keep, out = [], []
    for p in range(len(O)):
        if absorbed[p]:
            continue
        later = np.nonzero(~absorbed[p + 1:] & (oc[p + 1:] == oc[p]))[0] + p + 1
        m = match_value(ob[p], ob[later], metric)
        took = later[~(m <= thr)]
        absorbed[took] = True
        owner[O[took]] = O[p]
        box = ob[p].copy()
        if mode == UNION and len(took):
            box = np.array([min(box[0], ob[took, 0].min()), min(box[1], ob[took, 1].min()),
                            max(box[2], ob[took, 2].max()), max(box[3], ob[took, 3].max())], np.float32)
        keep.append(int(O[p]))
        out.append(box)
    if max_det is not None and len(keep) > max_det:
        best = set(sorted(keep, key=lambda i: (scores[i].item(), views[i], anchors[i]), reverse=True)[:max_det])
        sel = [n for n, i in enumerate(keep) if i in best]
        keep, out = [keep[n] for n in sel], [out[n] for n in sel]
    res = (np.array(keep, np.int64), np.array(out, np.float32).reshape(-1, 4))
    return res + (owner,) if owners else res
