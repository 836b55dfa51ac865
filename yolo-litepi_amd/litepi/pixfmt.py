"""Pixel formats of the frames the pipeline accepts (include/litepi.h ``lp_frame_format``) and a host restatement of the
device's NV12 -> BGR conversion, for what touches pixels on the host (the ``--save_viz`` overlays).

An NV12 host frame is a C-contiguous ``uint8`` array of shape ``(H * 3 // 2, W)`` -- cv2's convention: ``H`` rows of luma, then
``H / 2`` rows of interleaved ``U, V`` bytes, one pair per 2 x 2 block of pixels.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

PIXEL_FORMATS = {"bgr": 0, "nv12": 1}            # lp_pixfmt
CSC_MATRICES = {"bt601": 0, "bt709": 1}          # lp_csc

# CY, CVR, CUG, CVG, CUB: round(c * 2^20) of the limited-range coefficients (bt601 are cv2's constants)
_COEF = {"bt601": (1220542, 1673527, 409993, 852492, 2116026),
         "bt709": (1220542, 1880097, 223347, 558891, 2214593)}


def nv12_frame_hw(shape) -> Tuple[int, int]:
    """(H, W) of an NV12 host frame of the given array shape; ValueError for a shape that is not (H * 3 // 2, W), H and W even."""
    if len(shape) != 2 or shape[0] % 3 != 0 or shape[0] == 0 or shape[1] == 0 or (shape[0] // 3 * 2) % 2 != 0 or shape[1] % 2 != 0:
        raise ValueError(f"expected an NV12 uint8 frame of shape (H * 3 // 2, W) with even H and W, got shape {tuple(shape)}")
    return shape[0] // 3 * 2, shape[1]


def nv12_to_bgr(frame: np.ndarray, matrix: str = "bt601") -> np.ndarray:
    """(H * 3 // 2, W) NV12 -> (H, W, 3) BGR with the device's arithmetic: limited range, 20-bit fixed point, floor shift."""
    a = np.asarray(frame, dtype=np.uint8)
    H, W = nv12_frame_hw(a.shape)
    cy, cvr, cug, cvg, cub = _COEF[matrix]
    y = np.maximum(a[:H].astype(np.int32) - 16, 0) * cy + (1 << 19)
    uv = a[H:].reshape(H // 2, W // 2, 2).astype(np.int32) - 128
    u = np.repeat(np.repeat(uv[..., 0], 2, axis=0), 2, axis=1)
    v = np.repeat(np.repeat(uv[..., 1], 2, axis=0), 2, axis=1)
    out = np.empty((H, W, 3), np.uint8)
    out[..., 0] = np.clip((y + cub * u) >> 20, 0, 255)
    out[..., 1] = np.clip((y - cvg * v - cug * u) >> 20, 0, 255)
    out[..., 2] = np.clip((y + cvr * v) >> 20, 0, 255)
    return out
