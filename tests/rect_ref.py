"""Reference of a rectangular detector input (include/litepi.h lp_letterbox_geometry): the reference's
``letterbox(img, (SH, SW))`` (src/tt100k/pipeline/e2e.py:66-86) restated for a ``(rows, columns)`` shape, and the detect
path on top of it.  The resize is ``oracle.postprocess_ref.resize_linear_u8``, the forward
``oracle.ncnn_ref.run_graph`` and the decode ``oracle.postprocess_ref.postprocess``: all three are shape-generic.

TEST INFRASTRUCTURE ONLY: nothing here is imported by the product."""
from __future__ import annotations

import numpy as np

from oracle import postprocess_ref as P


def letterbox_geometry(det_h: int, det_w: int, h: int, w: int) -> dict:
    """e2e.py:72-83 with new_shape = (det_h, det_w), in Python doubles; round() is round-half-to-even.  The three floats are
    what the library stores: the doubles rounded to float32."""
    r = min(det_h / h, det_w / w)
    new_w, new_h = int(round(w * r)), int(round(h * r))
    dw, dh = (det_w - new_w) / 2, (det_h - new_h) / 2
    return dict(ratio=np.float32(r), pad_w=np.float32(dw), pad_h=np.float32(dh), new_w=new_w, new_h=new_h,
                top=int(round(dh - 0.1)), left=int(round(dw - 0.1)), bottom=int(round(dh + 0.1)), right=int(round(dw + 0.1)),
                r=r, dw=dw, dh=dh)


def letterbox(img: np.ndarray, det_h: int, det_w: int, color: int = 114):
    """e2e.py:66-86 on uint8 HxWx3 -> (uint8 [det_h, det_w, 3], ratio, (dw, dh)); bars of 114"""
    h, w = img.shape[:2]
    g = letterbox_geometry(det_h, det_w, h, w)
    if (w, h) != (g["new_w"], g["new_h"]):
        img = P.resize_linear_u8(img, g["new_w"], g["new_h"])
    out = np.full((det_h, det_w, 3), color, np.uint8)
    assert g["top"] + g["new_h"] + g["bottom"] == det_h and g["left"] + g["new_w"] + g["right"] == det_w
    out[g["top"]:g["top"] + g["new_h"], g["left"]:g["left"] + g["new_w"]] = img
    return out, g["r"], (g["dw"], g["dh"])


def to_input(bgr_batch: np.ndarray):
    """uint8 BGR [B, SH, SW, 3] -> the graph's input: RGB, x * (1/255) in fp32, NCHW (e2e.py:222-238)"""
    import torch
    return torch.from_numpy(bgr_batch[..., ::-1].astype(np.float32) * np.float32(1 / 255.0)).permute(0, 3, 1, 2).contiguous()


def out0(layers, bgr_batch: np.ndarray) -> np.ndarray:
    """oracle forward of already letterboxed images: fp32 out0 [B, 4 + nc, A]"""
    from oracle import ncnn_ref
    return ncnn_ref.run_graph(layers, to_input(bgr_batch))["out0"].numpy()


def detect(layers, img: np.ndarray, det_h: int, det_w: int, conf: float, iou: float):
    """letterbox -> graph -> postprocess of one image: (boxes in image pixels, scores, classes)"""
    lb, r, pad = letterbox(img, det_h, det_w)
    return P.postprocess(out0(layers, lb[None])[0], img.shape[:2], r, pad, conf, iou)


def anchor_table(det_h: int, det_w: int, strides=(8, 16, 32)):
    """the row-major grid of the Detect head: [2, A] points (x + 0.5, y + 0.5) and [A] strides, levels in order"""
    pts, st = [], []
    for s in strides:
        for y in range(det_h // s):
            for x in range(det_w // s):
                pts.append((x + 0.5, y + 0.5))
                st.append(float(s))
    return np.array(pts, np.float32).T, np.array(st, np.float32)
