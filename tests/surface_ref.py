"""Test helpers of the decoder-surface front door (include/litepi.h ``lp_surface``): the P010 widening / narrowing the contract
states, and a packer that lays a tight NV12 frame out as two planes with a pitch and a leading byte offset each.

The colour oracle stays tests/pixfmt_ref.py (imported, not edited): a P010 surface converts to what its narrowed NV12 frame
converts to.
"""
import numpy as np

import pixfmt_ref as R

SAMPLE_BYTES = {"nv12": 1, "p010": 2}


def widen(frame, rng=None, low=None):
    """Tight 8-bit frame [rows, W] -> uint16 samples ``byte << 8 | low byte``: random low bytes from rng, else the constant
    `low` (default 0, which is what a P010 decoder leaves in the 6 unused bits plus two zero value bits)."""
    f = np.asarray(frame, dtype=np.uint8).astype(np.uint16) << 8
    if rng is not None:
        return f | rng.integers(0, 256, f.shape, dtype=np.uint16)
    return f | np.uint16(low or 0)


def narrow(samples):
    """uint16 samples -> the bytes the contract reads: the HIGH byte of each, whatever the low byte holds."""
    return (np.asarray(samples, dtype=np.uint16) >> 8).astype(np.uint8)


def surface_bgr(frame, pixfmt="nv12", matrix="bt601"):
    """The BGR frame a surface holding `frame` converts to: `frame` is tight [H * 3 // 2, W], uint8 for NV12, uint16 for P010."""
    return R.nv12_to_bgr(narrow(frame) if pixfmt == "p010" else np.asarray(frame, dtype=np.uint8), matrix)


def pack_plane(rows, pitch=0, offset=0, tail=0, fill=0xEE):
    """[n, row_samples] samples (uint8 or uint16) -> (bytes, offset): a 1-D uint8 buffer holding the rows `pitch` bytes apart
    (0 = tight) from byte `offset` on, `tail` spare bytes behind the last row's samples; every byte that is no sample is `fill`.
    The buffer ends with the last row's samples plus `tail`: a reader that passes pitch x rows runs off the allocation."""
    rows = np.ascontiguousarray(rows)
    n, row_bytes = rows.shape[0], rows.shape[1] * rows.itemsize
    pitch = pitch or row_bytes
    assert pitch >= row_bytes and offset >= 0
    buf = np.full(offset + (n - 1) * pitch + row_bytes + tail, fill, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[offset:], shape=(n, row_bytes), strides=(pitch, 1))
    view[...] = rows.view(np.uint8).reshape(n, row_bytes)
    return buf, offset


def split_planes(frame):
    """Tight frame [H * 3 // 2, W] -> (luma rows [H, W], chroma rows [H / 2, W])."""
    rows = frame.shape[0]
    H = rows // 3 * 2
    return frame[:H], frame[H:]
