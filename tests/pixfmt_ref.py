"""Test oracle of the NV12 -> BGR conversion (include/litepi.h ``lp_frame_format``) and helpers that build NV12 inputs.

The oracle is the published formula restated in NumPy ``int64`` -- independent of the product's ``litepi/pixfmt.py`` and of the
kernel: limited-range YCbCr -> 8-bit BGR in 20-bit fixed point, ``>>`` an arithmetic (floor) shift.  Equality with OpenCV's
``cvtColor(COLOR_YUV2BGR_NV12)`` itself is not pinned (cv2 is not a dependency); the contract is this formula.
"""
import numpy as np

# CY, CVR, CUG, CVG, CUB = round(c * 2^20) of 1.164 / 1.596 / 0.391 / 0.813 / 2.018 and 1.164 / 1.793 / 0.213 / 0.533 / 2.112
COEF = {"bt601": (1220542, 1673527, 409993, 852492, 2116026),
        "bt709": (1220542, 1880097, 223347, 558891, 2214593)}

# (Y, U, V) -> (B, G, R)
WORKED = {"bt601": [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((0, 0, 0), (0, 154, 0)),
                    ((255, 255, 255), (255, 125, 255)), ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)),
                    ((41, 240, 110), (255, 0, 0))],
          "bt709": [((0, 0, 0), (0, 95, 0)), ((255, 255, 255), (255, 183, 255)), ((81, 90, 240), (0, 24, 255)),
                    ((200, 255, 0), (255, 255, 0))]}


def yuv_to_bgr(Y, U, V, matrix="bt601", return_terms=False):
    """Element-wise conversion of equally shaped (or broadcastable) Y, U, V arrays -> uint8 [..., 3] in B, G, R order.
    return_terms: also the list of every int64 intermediate (for the int32-safety check)."""
    cy, cvr, cug, cvg, cub = COEF[matrix]
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    u, v = U - 128, V - 128
    y = np.maximum(Y - 16, 0) * cy
    h = 1 << 19
    r_ = y + h + cvr * v
    g_ = y + h - cvg * v - cug * u
    b_ = y + h + cub * u
    b_, g_, r_ = np.broadcast_arrays(b_, g_, r_)
    out = np.stack([np.clip(b_ >> 20, 0, 255), np.clip(g_ >> 20, 0, 255), np.clip(r_ >> 20, 0, 255)], axis=-1).astype(np.uint8)
    if return_terms:
        return out, [y, y + h, cvr * v, cvg * v, cug * u, cub * u, y + h - cvg * v, r_, g_, b_]
    return out


def planes_to_bgr(y_plane, uv_plane, matrix="bt601"):
    """Y plane [H, W] and interleaved UV plane [H/2, W] -> BGR [H, W, 3]."""
    H, W = y_plane.shape
    uv = np.asarray(uv_plane).reshape(H // 2, W // 2, 2)
    U = np.repeat(np.repeat(uv[..., 0], 2, axis=0), 2, axis=1)
    V = np.repeat(np.repeat(uv[..., 1], 2, axis=0), 2, axis=1)
    return yuv_to_bgr(y_plane, U, V, matrix)


def nv12_to_bgr(frame, matrix="bt601"):
    """Tight NV12 host frame [H * 3 // 2, W] -> BGR [H, W, 3]."""
    rows, W = frame.shape
    H = rows // 3 * 2
    return planes_to_bgr(frame[:H], frame[H:], matrix)


def bgr_to_nv12(img):
    """Forward helper for building inputs (no parity claim): BT.601 limited-range RGB -> YCbCr in float64, chroma averaged
    over each 2 x 2 block, rounded.  [H, W, 3] BGR (even H, W) -> tight NV12 [H * 3 // 2, W]."""
    H, W = img.shape[:2]
    assert H % 2 == 0 and W % 2 == 0
    b, g, r = (img[..., k].astype(np.float64) for k in range(3))
    y = 16.0 + 0.256788 * r + 0.504129 * g + 0.097906 * b
    u = 128.0 - 0.148223 * r - 0.290993 * g + 0.439216 * b
    v = 128.0 + 0.439216 * r - 0.367788 * g - 0.071427 * b
    sub = lambda p: p.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))   # noqa: E731
    out = np.empty((H * 3 // 2, W), np.uint8)
    out[:H] = np.clip(np.rint(y), 0, 255)
    uv = np.stack([sub(u), sub(v)], axis=-1)
    out[H:] = np.clip(np.rint(uv), 0, 255).reshape(H // 2, W)
    return out


def pack_frames(frames, pitch=0, uv_offset=0, frame_stride=0, fill=0xEE):
    """Tight NV12 frames of ONE size -> the bytes of the same frames in a pitched layout (1-D uint8): rows `pitch` bytes
    apart, the UV plane `uv_offset` bytes behind the first Y byte, frames `frame_stride` bytes apart; every byte that is not
    a sample holds `fill`.  Returns (bytes, uv_offset, frame_bytes, frame_stride) with the zeros resolved."""
    rows, W = frames[0].shape
    H = rows // 3 * 2
    pitch = pitch or W
    uv_offset = uv_offset or pitch * H
    frame_bytes = uv_offset + pitch * (H // 2)
    frame_stride = frame_stride or frame_bytes
    assert pitch >= W and uv_offset >= pitch * H and frame_stride >= frame_bytes
    n = len(frames)
    buf = np.full((n - 1) * frame_stride + frame_bytes, fill, np.uint8)
    for i, f in enumerate(frames):
        assert f.shape == (rows, W)
        base = i * frame_stride
        yv = np.lib.stride_tricks.as_strided(buf[base:], shape=(H, W), strides=(pitch, 1))
        yv[...] = f[:H]
        uvv = np.lib.stride_tricks.as_strided(buf[base + uv_offset:], shape=(H // 2, W), strides=(pitch, 1))
        uvv[...] = f[H:]
    return buf, uv_offset, frame_bytes, frame_stride


def all_yuv_frames():
    """64 tight NV12 frames of 512 x 512 in which every one of the 2^24 (Y, U, V) combinations occurs exactly once: a frame
    has 65536 blocks of 2 x 2 pixels; frame f takes the 1024 chroma pairs p = U * 256 + V = 1024 f + k, and the 256 luma
    values of pair p fill 64 consecutive blocks."""
    frames = []
    ys = np.arange(256, dtype=np.uint8).reshape(64, 2, 2)            # 64 blocks x (2 x 2) luma values
    for f in range(64):
        pairs = np.arange(1024 * f, 1024 * (f + 1))                   # chroma pair index = U * 256 + V
        blk_uv = np.repeat(pairs, 64)                                 # 65536 blocks, pair-major
        blk_y = np.tile(ys, (1024, 1, 1))                             # [65536, 2, 2]
        Y = blk_y.reshape(256, 256, 2, 2).transpose(0, 2, 1, 3).reshape(512, 512)
        uv = np.stack([blk_uv >> 8, blk_uv & 255], axis=-1).astype(np.uint8).reshape(256, 512)
        frames.append(np.concatenate([Y, uv], axis=0))
    return frames
