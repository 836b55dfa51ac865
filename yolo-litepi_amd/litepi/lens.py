"""Remap tables for mapped views (include/litepi.h "mapped views"; Engine.map_add, HybridPipeline(view_maps=...)).

A table is xy [S, S, 2] float32: for view pixel (row j, column i) the frame position (x, y) it shows, in pixel-index
coordinates with pixel centres at integers (cv2.remap's convention).  The builders here are a convenience, NumPy only, float64
inside and cast to float32 at the end; the library's contract starts at the table, and any other source of tables (cv2's
initUndistortRectifyMap, a calibration tool, a mirror) serves as well.

The virtual camera of the pinhole builders is an S x S pinhole picture with horizontal field of view `hfov` (degrees), focal
length f = (S / 2) / tan(hfov / 2) pixels and its principal point at the view's centre ((S - 1) / 2, (S - 1) / 2).  Camera axes:
x right, y down, z forward.  The view direction is the lens axis turned by R = Ry(yaw) Rx(pitch) Rz(roll), angles in degrees:
yaw > 0 looks right, pitch > 0 looks up, roll > 0 turns the picture clockwise.  A ray the lens model cannot show (behind a
pinhole lens) gets the position (-3, -3): outside every frame, so the pixel is border grey.
"""
from __future__ import annotations

import numpy as np

OUTSIDE = -3.0   # a position outside every frame (the table clamps to -2; taps there are border grey)


def crop_map(S: int, x0: float, y0: float, scale: float = 1.0) -> np.ndarray:
    """The square window of S * scale frame pixels a side whose first pixel is (x0, y0), resampled to S x S:
    x = x0 + (i + 0.5) * scale - 0.5, y likewise.  With scale 1 view pixel (j, i) is frame position (x0 + i, y0 + j): an
    integer (x0, y0) copies frame[y0 : y0 + S, x0 : x0 + S]."""
    i = np.arange(S, dtype=np.float64)
    x = x0 + (i + 0.5) * scale - 0.5
    y = y0 + (i + 0.5) * scale - 0.5
    xy = np.empty((S, S, 2), dtype=np.float64)
    xy[..., 0] = x[None, :]
    xy[..., 1] = y[:, None]
    return xy.astype(np.float32)


def rotation(yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0) -> np.ndarray:
    """R = Ry(yaw) Rx(pitch) Rz(roll), degrees: the lens-frame direction of a view-frame ray d is R @ d."""
    a, b, c = np.radians([yaw, pitch, roll]).astype(np.float64)
    ry = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(b), -np.sin(b)], [0.0, np.sin(b), np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0.0], [np.sin(c), np.cos(c), 0.0], [0.0, 0.0, 1.0]])
    return ry @ rx @ rz


def view_rays(S: int, yaw: float, pitch: float, roll: float, hfov: float) -> np.ndarray:
    """The lens-frame directions [S, S, 3] (not normalised) of the virtual pinhole camera's pixels."""
    if not 0.0 < hfov < 180.0:
        raise ValueError(f"hfov {hfov} outside (0, 180) degrees")
    f = (S / 2.0) / np.tan(np.radians(float(hfov)) / 2.0)
    c = (S - 1) / 2.0
    i = np.arange(S, dtype=np.float64) - c
    d = np.empty((S, S, 3), dtype=np.float64)
    d[..., 0] = i[None, :]
    d[..., 1] = i[:, None]
    d[..., 2] = f
    return d @ rotation(yaw, pitch, roll).T


def _intrinsics(K):
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError(f"K is a 3 x 3 camera matrix (got {K.shape})")
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def _finish(u, v, ok) -> np.ndarray:
    xy = np.stack([np.where(ok, u, OUTSIDE), np.where(ok, v, OUTSIDE)], axis=-1)
    return xy.astype(np.float32)


def pinhole_from_brown(S: int, K, dist=(), yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0, hfov: float = 90.0) -> np.ndarray:
    """A rectified pinhole view out of a frame taken through a lens of OpenCV's Brown-Conrady model: camera matrix K and
    dist = (k1, k2, p1, p2[, k3]) (missing coefficients are 0)."""
    fx, fy, cx, cy = _intrinsics(K)
    k = np.zeros(5, dtype=np.float64)
    dist = np.asarray(dist, dtype=np.float64).reshape(-1)
    if len(dist) > 5:
        raise ValueError("dist holds at most k1, k2, p1, p2, k3")
    k[:len(dist)] = dist
    k1, k2, p1, p2, k3 = k
    d = view_rays(S, yaw, pitch, roll, hfov)
    ok = d[..., 2] > 1e-9
    z = np.where(ok, d[..., 2], 1.0)
    x, y = d[..., 0] / z, d[..., 1] / z
    r2 = x * x + y * y
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return _finish(fx * xd + cx, fy * yd + cy, ok)


def pinhole_from_fisheye(S: int, K, D=(), yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0, hfov: float = 90.0) -> np.ndarray:
    """A rectified pinhole view out of a frame taken through a fisheye lens of OpenCV's equidistant model (cv2.fisheye): camera
    matrix K and D = (k1, k2, k3, k4) (missing coefficients are 0): theta_d = theta (1 + k1 theta^2 + ... + k4 theta^8).  Rays
    up to 180 degrees off the lens axis are shown."""
    fx, fy, cx, cy = _intrinsics(K)
    k = np.zeros(4, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    if len(D) > 4:
        raise ValueError("D holds at most k1, k2, k3, k4")
    k[:len(D)] = D
    d = view_rays(S, yaw, pitch, roll, hfov)
    rxy = np.hypot(d[..., 0], d[..., 1])
    theta = np.arctan2(rxy, d[..., 2])
    t2 = theta * theta
    theta_d = theta * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    on_axis = rxy < 1e-12
    s = np.where(on_axis, 0.0, theta_d / np.where(on_axis, 1.0, rxy))
    ok = np.ones(theta.shape, dtype=bool)
    return _finish(fx * s * d[..., 0] + cx, fy * s * d[..., 1] + cy, ok)


def pinhole_from_equirect(S: int, H: int, W: int, yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0, hfov: float = 90.0) -> np.ndarray:
    """A perspective view out of an H x W equirectangular panorama (360 x 180 degrees; its centre column looks forward, its
    top row up): x = (lon / 360 + 0.5) * W - 0.5 wrapped into [-0.5, W - 0.5), y = (lat / 180 + 0.5) * H - 0.5 with the
    latitude growing downwards.  The library's pixel rule does not wrap: a view across the panorama's seam has one column pair
    blended with border grey; roll the panorama (np.roll) so that the views stay clear of the seam."""
    d = view_rays(S, yaw, pitch, roll, hfov)
    lon = np.arctan2(d[..., 0], d[..., 2])
    lat = np.arcsin(np.clip(d[..., 1] / np.linalg.norm(d, axis=-1), -1.0, 1.0))
    u = (lon / (2.0 * np.pi) + 0.5) * W - 0.5
    u = np.mod(u + 0.5, float(W)) - 0.5
    v = (lat / np.pi + 0.5) * H - 0.5
    return _finish(u, v, np.ones(u.shape, dtype=bool))
