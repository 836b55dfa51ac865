"""CPU oracle of scaled views (test infrastructure only; include/litepi.h "scaled views" states the semantics).

A view is an (x, y, w, h) source window of a frame, x = -1 for the whole frame.  The view's pixels are
``postprocess_ref.letterbox(frame[y:y+h, x:x+w], S)``; its geometry is the letterbox geometry of an h x w image with the
pads moved by the window's origin.  Candidates, merge and the pipeline are those of ``tiling_ref``.  Nothing here imports
from the product.
"""
from typing import List, Sequence, Tuple

import numpy as np
import torch

import tiling_ref as T
from oracle import ncnn_ref, postprocess_ref as P

FULL = (-1, -1, 0, 0)


def view_axis(L: int, tile: int, overlap: int) -> Tuple[List[int], int]:
    """origins and the common side of one axis of the window grid"""
    if L <= tile:
        return [0], L
    step = tile - overlap
    n = 1 + -(-(L - tile) // step)
    return [min(k * step, L - tile) for k in range(n)], tile


def view_grid(tile: int, H: int, W: int, overlap: int = 0, full_frame: bool = True) -> List[Tuple[int, int, int, int]]:
    if tile < 16 or not 0 <= overlap < tile:
        raise ValueError(f"tile {tile} / overlap {overlap}")
    xs, sw = view_axis(W, tile, overlap)
    ys, sh = view_axis(H, tile, overlap)
    views = []
    if len(xs) * len(ys) == 1 or full_frame:
        views.append((-1, -1, W, H))
    if len(xs) * len(ys) > 1:
        views += [(x, y, sw, sh) for y in ys for x in xs]
    return views


def window(view, H: int, W: int) -> Tuple[int, int, int, int]:
    """the window a view covers on an H x W frame; ValueError for one the frame does not hold"""
    x, y, w, h = FULL if isinstance(view, str) and view == "full" else (int(c) for c in view)
    if x == -1:
        return 0, 0, W, H
    if x < 0 or y < 0 or w < 16 or h < 16 or x + w > W or y + h > H:
        raise ValueError(f"window {(x, y, w, h)} on a {W}x{H} frame")
    return x, y, w, h


def view_geometry(S: int, H: int, W: int, view):
    """dict(ratio, pad_w, pad_h as float32; new_w, new_h, top, left) -- Python doubles, rounded once"""
    x, y, w, h = window(view, H, W)
    r, (nw, nh), (dw, dh), (top, _, left, _) = P.letterbox_params(h, w, S)
    return dict(ratio=np.float32(r), pad_w=np.float32(dw - r * x), pad_h=np.float32(dh - r * y), new_w=nw, new_h=nh, top=top, left=left)


def make_view(img: np.ndarray, S: int, view):
    """(view uint8 [S,S,3], ratio, (pad_w, pad_h)) with ratio / pads as doubles"""
    H, W = img.shape[:2]
    x, y, w, h = window(view, H, W)
    lb, r, (dw, dh) = P.letterbox(np.ascontiguousarray(img[y:y + h, x:x + w]), S)
    assert lb.shape == (S, S, 3)
    return lb, r, (dw - r * x, dh - r * y)


def make_views(img: np.ndarray, S: int, views: Sequence):
    return [make_view(img, S, v) for v in views]


class CpuViewsPipeline(T.CpuTiledPipeline):
    """CpuTiledPipeline with the frame seen through a list of scaled views."""

    @torch.no_grad()
    def view_candidates(self, img: np.ndarray, views: Sequence, conf: float):
        bs, ss, cs, vs, an = [], [], [], [], []
        for k, (v, r, pad) in enumerate(make_views(img, self.S, views)):
            x, _, _ = P.preprocess(v, self.S)   # an S x S view: the letterbox is the identity
            out0 = ncnn_ref.run_graph(self.layers, torch.from_numpy(x))["out0"].numpy()[0]
            b, s, c, a = T.view_candidates(out0, img.shape[:2], r, pad, conf)
            bs.append(b); ss.append(s); cs.append(c); an.append(a); vs.append(np.full(len(a), k, np.int64))
        return (np.concatenate(bs).reshape(-1, 4), np.concatenate(ss), np.concatenate(cs), np.concatenate(vs), np.concatenate(an))

    def run_views(self, img, views, conf=0.5, iou=0.45, min_area=100):
        from oracle import shufflenet_ref
        b, s, c, v, a = self.view_candidates(img, views, conf)
        k = T.merge(b, s, c, v, a, iou)
        boxes, scores, det_cls = b[k], s[k], c[k]
        num = len(boxes)
        h, w = img.shape[:2]
        rects, valid = P.roi_rects(boxes, h, w, min_area)
        rois = [img[y1:y2, x1:x2] for x1, y1, x2, y2 in rects]
        ids = shufflenet_ref.predict_batch(self.cls, rois, self.cls_input)[0] if (rois and self.cls is not None) else []
        boxes, scores, det_cls = boxes[valid], scores[valid], det_cls[valid]
        res = [{"bbox": tuple(boxes[i].astype(int)), "det_class": int(det_cls[i]), "det_conf": float(scores[i]),
                "cls_class": int(ids[i]) if i < len(ids) else -1} for i in range(len(boxes))]
        return res, num
