"""CPU oracle of mapped views (test infrastructure only; include/litepi.h "mapped views" states the three rules).

``fixed`` / ``render`` / ``map_box`` restate the table, pixel and box rules in NumPy -- the box rule in np.float32 operations one
at a time, so that every operation is rounded on its own as the library's fp32 code is.  ``CASES`` builds the maps the tests
share, ``boxes`` their view boxes, and ``CpuMappedPipeline`` is the end-to-end oracle: render, oracle detector, decode as a crop
of an S x S image, ``map_box``, frame NMS, ROI, classifier (views_ref / tiling_ref).  Nothing here imports from the product.
"""
from typing import Dict, Sequence

import numpy as np
import torch

import tiling_ref as T
import views_ref as V
from oracle import ncnn_ref, postprocess_ref as P

F = np.float32
BORDER = 114


# ---------------------------------------------------------------------------- the three rules
def fixed(xy: np.ndarray, H: int, W: int) -> np.ndarray:
    """xy [S, S, 2] float32 -> int32 with 5 fractional bits: rint(min(max(x, -2), L + 1) * 32) in doubles, half to even"""
    xy = np.asarray(xy, dtype=np.float32)
    if np.isnan(xy).any():
        raise ValueError("NaN in a map")
    x = np.minimum(np.maximum(xy[..., 0].astype(np.float64), -2.0), float(W) + 1.0)
    y = np.minimum(np.maximum(xy[..., 1].astype(np.float64), -2.0), float(H) + 1.0)
    return np.stack([np.rint(x * 32.0), np.rint(y * 32.0)], axis=-1).astype(np.int32)


def render(fx: np.ndarray, frame: np.ndarray) -> np.ndarray:
    """the view [S, S, 3] of a BGR frame [H, W, 3] through a fixed table, in integers"""
    H, W = frame.shape[:2]
    f = fx.astype(np.int64)
    ix, ax = f[..., 0] >> 5, f[..., 0] & 31
    iy, ay = f[..., 1] >> 5, f[..., 1] & 31

    def tap(r, c):
        ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        px = frame[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)].astype(np.int64)
        return np.where(ok[..., None], px, BORDER)

    wx0, wx1, wy0, wy1 = (32 - ax)[..., None], ax[..., None], (32 - ay)[..., None], ay[..., None]
    acc = tap(iy, ix) * wx0 * wy0 + tap(iy, ix + 1) * wx1 * wy0 + tap(iy + 1, ix) * wx0 * wy1 + tap(iy + 1, ix + 1) * wx1 * wy1 + 512
    return (acc >> 10).astype(np.uint8)


def _cell(u: np.ndarray, S: int):
    t = u - F(0.5)
    i = np.clip(np.floor(t), 0, S - 2).astype(np.int64)
    return i, t - i.astype(np.float32)


def _point(comp: np.ndarray, S: int, u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """one component ([S, S] int32) of the frame positions of the view points (u, v), float32 arrays"""
    i, fu = _cell(u, S)
    j, fv = _cell(v, S)

    def X(r, c):
        return comp[r, c].astype(np.float32) * F(0.03125)

    d0 = X(j, i + 1) - X(j, i)
    top = X(j, i) + fu * d0
    d1 = X(j + 1, i + 1) - X(j + 1, i)
    bot = X(j + 1, i) + fu * d1
    d2 = bot - top
    s = top + fv * d2
    out = s + F(0.5)
    assert out.dtype == np.float32
    return out


def map_box(fx: np.ndarray, H: int, W: int, boxes) -> np.ndarray:
    """view boxes [n, 4] -> frame boxes [n, 4] float32: the bounding box of the four corners and the four edge midpoints
    through the table, clipped to the frame"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    S = fx.shape[0]
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    xm, ym = (x1 + x2) * F(0.5), (y1 + y2) * F(0.5)
    us = np.stack([x1, xm, x2, x1, x2, x1, xm, x2])
    vs = np.stack([y1, y1, y1, ym, ym, y2, y2, y2])
    px = _point(fx[..., 0], S, us, vs)
    py = _point(fx[..., 1], S, us, vs)
    out = np.stack([px.min(axis=0), py.min(axis=0), px.max(axis=0), py.max(axis=0)], axis=1)
    hi = np.array([W, H, W, H], dtype=np.float32)
    return np.minimum(np.maximum(out, F(0.0)), hi).astype(np.float32)


# ---------------------------------------------------------------------------- the maps of the tests
def crop(S: int, x0: float, y0: float, scale: float = 1.0) -> np.ndarray:
    i = np.arange(S, dtype=np.float64)
    xy = np.empty((S, S, 2))
    xy[..., 0] = (x0 + (i + 0.5) * scale - 0.5)[None, :]
    xy[..., 1] = (y0 + (i + 0.5) * scale - 0.5)[:, None]
    return xy.astype(np.float32)


def rotated(S: int, H: int, W: int, degrees: float, scale: float) -> np.ndarray:
    """the frame's centre region turned by `degrees`, `scale` frame pixels per view pixel"""
    c = (S - 1) / 2.0
    j, i = np.meshgrid(np.arange(S) - c, np.arange(S) - c, indexing="ij")
    a = np.radians(degrees)
    xy = np.empty((S, S, 2))
    xy[..., 0] = (W - 1) / 2.0 + scale * (np.cos(a) * i - np.sin(a) * j)
    xy[..., 1] = (H - 1) / 2.0 + scale * (np.sin(a) * i + np.cos(a) * j)
    return xy.astype(np.float32)


def barrel(S: int, H: int, W: int, k1: float, scale: float = None) -> np.ndarray:
    """x_d = c + (x - c)(1 + k1 r^2), r normalised to the view's half side: the view undoes a barrel lens"""
    c = (S - 1) / 2.0
    j, i = np.meshgrid((np.arange(S) - c) / (S / 2.0), (np.arange(S) - c) / (S / 2.0), indexing="ij")
    g = 1.0 + k1 * (i * i + j * j)
    half = min(H, W) / 2.0 if scale is None else scale * S / 2.0
    xy = np.empty((S, S, 2))
    xy[..., 0] = (W - 1) / 2.0 + half * i * g
    xy[..., 1] = (H - 1) / 2.0 + half * j * g
    return xy.astype(np.float32)


def cases(S: int, H: int, W: int) -> Dict[str, np.ndarray]:
    """the maps every test of the rules runs, by name"""
    rng = np.random.default_rng(S * 1000003 + H * 1009 + W)
    rnd = np.empty((S, S, 2))
    rnd[..., 0] = rng.uniform(-3.0, W + 2.0, (S, S))
    rnd[..., 1] = rng.uniform(-3.0, H + 2.0, (S, S))
    return {
        "crop": crop(S, 17, 3),                               # integer crops: inside where the frame holds them,
        "crop_corner": crop(S, W - S + 3, H - S + 2),         # ... and one that passes the right and the lower edge
        "half_pixel": crop(S, 10.5, 5.5),                     # ax = ay = 16 everywhere
        "rotation": rotated(S, H, W, 7.0, 1.3),
        "barrel": barrel(S, H, W, -0.3),
        "outside": crop(S, W + 50, H + 50),                   # wholly outside the frame
        "random": rnd.astype(np.float32),                     # uniform in [-3, W + 2] x [-3, H + 2]
        "last_pixel": crop(S, W - S, H - S),                  # the last view pixel is the frame's last pixel, fractions zero
        "last_pixel_frac": crop(S, W - S - 0.5, H - S - 0.25),   # ... and with ax = 16, ay = 8: its taps end on the last pixel
    }


def boxes(S: int, seed: int, n: int = 1000) -> np.ndarray:
    """n seeded view boxes in [0, S]: random ones, degenerate ones (x1 == x2, y1 == y2), ones touching 0 and S, the whole view"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, S, (n, 2, 2))
    b = np.concatenate([a.min(axis=1), a.max(axis=1)], axis=1).astype(np.float32)   # x1, y1, x2, y2
    b[0:40, 2] = b[0:40, 0]          # x1 == x2
    b[40:80, 3] = b[40:80, 1]        # y1 == y2
    b[80:120, 0] = 0.0               # touching 0
    b[120:160, 1] = 0.0
    b[160:200, 2] = S                # touching S
    b[200:240, 3] = S
    b[240] = (0.0, 0.0, S, S)
    b[241] = (0.0, 0.0, 0.0, 0.0)
    b[242] = (S, S, S, S)
    b[243:260] = np.round(b[243:260])   # on pixel borders
    return b


# ---------------------------------------------------------------------------- the end-to-end oracle
class CpuMappedPipeline(V.CpuViewsPipeline):
    """CpuViewsPipeline with the frame also seen through maps, behind the listed views."""

    @torch.no_grad()
    def mapped_candidates(self, img: np.ndarray, views: Sequence, maps: Sequence[np.ndarray], conf: float):
        H, W = img.shape[:2]
        parts = [self.view_candidates(img, views, conf)] if views else []
        for k, xy in enumerate(maps):
            fx = fixed(xy, H, W)
            x, _, _ = P.preprocess(render(fx, img), self.S)   # an S x S view: the letterbox is the identity
            out0 = ncnn_ref.run_graph(self.layers, torch.from_numpy(x))["out0"].numpy()[0]
            b, s, c, a = T.view_candidates(out0, (self.S, self.S), 1.0, (0.0, 0.0), conf)   # a crop of an S x S image
            parts.append((map_box(fx, H, W, b), s, c, np.full(len(a), len(views) + k, np.int64), a))
        return (np.concatenate([p[0] for p in parts]).reshape(-1, 4),) + tuple(np.concatenate([p[i] for p in parts]) for i in range(1, 5))

    def run_mapped(self, img, views, maps, conf=0.5, iou=0.45, min_area=100):
        from oracle import shufflenet_ref
        b, s, c, v, a = self.mapped_candidates(img, views, maps, conf)
        k = T.merge(b, s, c, v, a, iou)
        bx, scores, det_cls = b[k], s[k], c[k]
        num = len(bx)
        h, w = img.shape[:2]
        rects, valid = P.roi_rects(bx, h, w, min_area)
        rois = [img[y1:y2, x1:x2] for x1, y1, x2, y2 in rects]
        ids = shufflenet_ref.predict_batch(self.cls, rois, self.cls_input)[0] if (rois and self.cls is not None) else []
        bx, scores, det_cls = bx[valid], scores[valid], det_cls[valid]
        res = [{"bbox": tuple(bx[i].astype(int)), "det_class": int(det_cls[i]), "det_conf": float(scores[i]),
                "cls_class": int(ids[i]) if i < len(ids) else -1, "box": bx[i]} for i in range(len(bx))]
        return res, num
