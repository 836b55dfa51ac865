"""Decoder surfaces (include/litepi.h ``lp_surface``): one decoded frame where the decoder left it -- a device address and a
pitch per plane -- and the helpers that turn them into the C records ``Engine.run_surfaces_device`` passes on.

Nothing here touches the GPU: a ``Surface`` is four integers and two addresses, ``surfaces_check`` is ``lp_surfaces_check``
(pure host), and ``surface_from_tensors`` only reads a tensor's address, strides and dtype.  Anything malformed is a
``ValueError`` here or ``LitepiError(LP_ERR_ARG)`` from the library, never a silent reading.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Sequence, Tuple

from . import _ffi
from ._ffi import LpSurface, LpSurfaceFormat, check
from .pixfmt import CSC_MATRICES

SURFACE_FORMATS = {"nv12": _ffi.LP_SURF_NV12, "p010": _ffi.LP_SURF_P010}
SAMPLE_BYTES = {"nv12": 1, "p010": 2}


def _int(name: str, v) -> int:
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"surface {name} must be an integer, got {v!r}")
    return int(v)


@dataclass(frozen=True)
class Surface:
    """One decoded frame: DEVICE addresses of the luma rows and of the interleaved chroma rows (U first), the luma size in
    pixels (both even) and the bytes per row of each plane (0 = tight)."""
    y_ptr: int
    uv_ptr: int
    height: int
    width: int
    pitch_y: int = 0
    pitch_uv: int = 0

    def __post_init__(self):
        for name in ("y_ptr", "uv_ptr", "height", "width", "pitch_y", "pitch_uv"):
            object.__setattr__(self, name, _int(name, getattr(self, name)))
        # what a C record cannot even hold is refused here; every rule of the header is the library's (LP_ERR_ARG)
        if not (0 <= self.y_ptr < 2 ** 64 and 0 <= self.uv_ptr < 2 ** 64):
            raise ValueError("a plane address is an unsigned 64-bit integer")
        for name in ("height", "width", "pitch_y", "pitch_uv"):
            if not -2 ** 31 <= getattr(self, name) < 2 ** 31:
                raise ValueError(f"surface {name} {getattr(self, name)} does not fit an int")


def surface_format(pixfmt: str = "nv12", matrix: str = "bt601") -> LpSurfaceFormat:
    if pixfmt not in SURFACE_FORMATS:
        raise ValueError(f"unknown surface pixel format {pixfmt!r} (one of {sorted(SURFACE_FORMATS)})")
    if matrix not in CSC_MATRICES:
        raise ValueError(f"unknown colour matrix {matrix!r} (one of {sorted(CSC_MATRICES)})")
    f = LpSurfaceFormat()
    f.pixfmt, f.matrix = SURFACE_FORMATS[pixfmt], CSC_MATRICES[matrix]
    return f


def surface_array(surfaces: Sequence[Surface]):
    """The host array of lp_surface records of a call."""
    surfaces = list(surfaces)
    if not surfaces:
        raise ValueError("a call needs at least one surface")
    arr = (LpSurface * len(surfaces))()
    for rec, s in zip(arr, surfaces):
        if not isinstance(s, Surface):
            raise ValueError(f"expected a Surface, got {type(s).__name__}")
        rec.plane[0], rec.plane[1] = s.y_ptr, s.uv_ptr
        rec.pitch[0], rec.pitch[1] = s.pitch_y, s.pitch_uv
        rec.height, rec.width = s.height, s.width
    return arr


def surfaces_check(surfaces: Sequence[Surface], pixfmt: str = "nv12", matrix: str = "bt601") -> None:
    """lp_surfaces_check: every rule of the surface calls that needs no handle; LitepiError(LP_ERR_ARG) names the first
    broken one.  Host only, no GPU needed."""
    lib = _ffi.load_library()
    f, arr = surface_format(pixfmt, matrix), surface_array(surfaces)
    check(lib, lib.lp_surfaces_check(C.byref(f), arr, len(arr)))


_TORCH_FORMATS = {"torch.uint8": "nv12", "torch.int16": "p010", "torch.uint16": "p010"}


def surface_from_tensors(y, uv) -> Tuple[Surface, str]:
    """(Surface, pixfmt) of two torch DEVICE tensors: y [H, W] and uv [H / 2, W / 2, 2] or [H / 2, W] (U first), rows
    ``stride(0)`` elements apart and contiguous inside a row.  uint8 tensors are NV12 planes, int16 / uint16 tensors P010
    planes.  The tensors stay the caller's: keep them alive and unwritten until the stream has passed the call."""
    fmts = []
    for name, t in (("y", y), ("uv", uv)):
        for attr in ("data_ptr", "stride", "element_size", "dtype", "shape"):
            if not hasattr(t, attr):
                raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
        if str(t.dtype) not in _TORCH_FORMATS:
            raise ValueError(f"{name}: dtype {t.dtype} is neither uint8 (NV12) nor int16 / uint16 (P010)")
        fmts.append(_TORCH_FORMATS[str(t.dtype)])
        if getattr(t, "is_cuda", None) is False:
            raise ValueError(f"{name}: a surface plane is device memory; this tensor is on {t.device}")
    if fmts[0] != fmts[1]:
        raise ValueError(f"y is {y.dtype} and uv is {uv.dtype}: both planes of a surface have one sample type")
    if y.dim() != 2:
        raise ValueError(f"y: expected [H, W], got {tuple(y.shape)}")
    H, W = int(y.shape[0]), int(y.shape[1])
    if uv.dim() == 3 and tuple(uv.shape) == (H // 2, W // 2, 2):
        inner = uv.stride(2) == 1 and uv.stride(1) == 2
    elif uv.dim() == 2 and tuple(uv.shape) == (H // 2, W):
        inner = uv.stride(1) == 1
    else:
        raise ValueError(f"uv: expected [{H // 2}, {W // 2}, 2] or [{H // 2}, {W}] for a {H}x{W} luma plane, got {tuple(uv.shape)}")
    if y.stride(1) != 1 or not inner:
        raise ValueError("the samples of a row must be contiguous (only stride(0) may exceed the row)")
    if y.stride(0) < W or uv.stride(0) < W:
        raise ValueError("rows overlap: stride(0) is below the row's samples")
    es = y.element_size()
    return Surface(y.data_ptr(), uv.data_ptr(), H, W, y.stride(0) * es, uv.stride(0) * es), fmts[0]
