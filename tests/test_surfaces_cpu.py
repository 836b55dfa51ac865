"""CPU tests of the decoder-surface front door (include/litepi.h lp_surface): lp_surfaces_check accepts and
refuses exactly the header's list, the ctypes mirrors match the header's records, the Python helpers raise before any handle
exists, the P010 helpers of tests/surface_ref.py, and the exported symbols.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surface_ref as S

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "litepi.h")
A = 0x7F0000001000   # a 4096-aligned "device address": the check never dereferences it


def _check(fmt=None, surfaces=(), B=None, null_fmt=False, null_surfaces=False):
    """lp_surfaces_check on raw field values (no Python-side validation) -> status"""
    from litepi import _ffi
    lib = _ffi.load_library()
    f = _ffi.LpSurfaceFormat()
    for k, v in (fmt or {}).items():
        if k == "reserved":
            f.reserved[v] = 1
        else:
            setattr(f, k, v)
    arr = (_ffi.LpSurface * max(1, len(surfaces)))()
    for rec, s in zip(arr, surfaces):
        rec.plane[0], rec.plane[1] = s.get("y", A), s.get("uv", A + (1 << 20))
        rec.pitch[0], rec.pitch[1] = s.get("pitch_y", 0), s.get("pitch_uv", 0)
        rec.height, rec.width = s.get("h", 4), s.get("w", 6)
        if "reserved" in s:
            rec.reserved[s["reserved"]] = 1
    rc = lib.lp_surfaces_check(None if null_fmt else C.byref(f), None if null_surfaces else arr, len(surfaces) if B is None else B)
    if rc != 0:
        assert len(lib.lp_last_error()) > 0
    return rc


NV12, P010 = dict(pixfmt=1), dict(pixfmt=2)

ACCEPTED = [
    ("tight NV12", NV12, [dict()]),
    ("tight P010", P010, [dict()]),
    ("bt709", dict(pixfmt=1, matrix=1), [dict()]),
    ("NV12 pitch == W", NV12, [dict(pitch_y=6, pitch_uv=6)]),
    ("NV12 unequal pitches", NV12, [dict(pitch_y=7, pitch_uv=256)]),
    ("NV12 odd addresses", NV12, [dict(y=A + 1, uv=A + 4099)]),
    ("P010 pitch == 2 W", P010, [dict(pitch_y=12, pitch_uv=12)]),
    ("P010 even address and pitch", P010, [dict(y=A + 2, uv=A + 4102, pitch_y=14, pitch_uv=256)]),
    ("the smallest frame", NV12, [dict(h=2, w=2)]),
    ("individual sizes", NV12, [dict(h=2, w=2), dict(h=720, w=1280, pitch_y=1280), dict(h=482, w=366)]),
    ("luma and chroma in one allocation", NV12, [dict(y=A, uv=A + 24)]),
]

REFUSED = [
    ("null fmt", dict(fmt=NV12, surfaces=[dict()], null_fmt=True)),
    ("null surfaces", dict(fmt=NV12, surfaces=[dict()], null_surfaces=True)),
    ("pixfmt 0", dict(fmt=dict(pixfmt=0), surfaces=[dict()])),
    ("pixfmt 3", dict(fmt=dict(pixfmt=3), surfaces=[dict()])),
    ("pixfmt -1", dict(fmt=dict(pixfmt=-1), surfaces=[dict()])),
    ("matrix 2", dict(fmt=dict(pixfmt=1, matrix=2), surfaces=[dict()])),
    ("matrix -1", dict(fmt=dict(pixfmt=1, matrix=-1), surfaces=[dict()])),
    ("format reserved word", dict(fmt=dict(pixfmt=1, reserved=5), surfaces=[dict()])),
    ("surface reserved word", dict(fmt=NV12, surfaces=[dict(), dict(reserved=3)])),
    ("B = 0", dict(fmt=NV12, surfaces=[dict()], B=0)),
    ("B < 0", dict(fmt=NV12, surfaces=[dict()], B=-2)),
    ("null luma plane", dict(fmt=NV12, surfaces=[dict(y=0)])),
    ("null chroma plane", dict(fmt=NV12, surfaces=[dict(), dict(uv=0)])),
    ("odd height", dict(fmt=NV12, surfaces=[dict(h=5)])),
    ("odd width", dict(fmt=NV12, surfaces=[dict(w=7)])),
    ("zero height", dict(fmt=NV12, surfaces=[dict(h=0)])),
    ("negative width", dict(fmt=NV12, surfaces=[dict(w=-6)])),
    ("NV12 luma pitch < W", dict(fmt=NV12, surfaces=[dict(pitch_y=5)])),
    ("NV12 chroma pitch < W", dict(fmt=NV12, surfaces=[dict(pitch_uv=4)])),
    ("P010 luma pitch < 2 W", dict(fmt=P010, surfaces=[dict(pitch_y=10)])),
    ("P010 chroma pitch < 2 W", dict(fmt=P010, surfaces=[dict(pitch_uv=6)])),
    ("negative luma pitch", dict(fmt=NV12, surfaces=[dict(pitch_y=-8)])),
    ("negative chroma pitch", dict(fmt=NV12, surfaces=[dict(pitch_uv=-256)])),
    ("P010 odd luma address", dict(fmt=P010, surfaces=[dict(y=A + 1)])),
    ("P010 odd chroma address", dict(fmt=P010, surfaces=[dict(uv=A + 4097)])),
    ("P010 odd luma pitch", dict(fmt=P010, surfaces=[dict(pitch_y=13)])),
    ("P010 odd chroma pitch", dict(fmt=P010, surfaces=[dict(pitch_uv=257)])),
]


@pytest.mark.parametrize("name,fmt,surfaces", ACCEPTED, ids=[a[0] for a in ACCEPTED])
def test_surfaces_check_accepts(name, fmt, surfaces):
    assert _check(fmt, surfaces) == 0


@pytest.mark.parametrize("name,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_surfaces_check_refuses(name, kw):
    from litepi._ffi import LP_ERR_ARG
    assert _check(**kw) == LP_ERR_ARG


def test_what_nv12_allows_p010_refuses_and_back():
    from litepi._ffi import LP_ERR_ARG
    odd = [dict(y=A + 1, pitch_y=13, pitch_uv=13, w=12)]
    assert _check(NV12, odd) == 0 and _check(P010, odd) == LP_ERR_ARG
    assert _check(NV12, [dict(pitch_y=6)]) == 0 and _check(P010, [dict(pitch_y=6)]) == LP_ERR_ARG   # W bytes: half a P010 row


# ---------------------------------------------------------------------------- the records
def _header_struct(name):
    text = open(HEADER).read()
    m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.rsplit(" ", 1)[0], decl.rsplit(" ", 1)[1]
        if "," in decl:   # "int height, width"
            typ = decl.split(" ", 1)[0]
            names = decl.split(" ", 1)[1]
        for n in names.split(","):
            n = n.strip()
            m2 = re.match(r"(\w+)\[(\d+)\]", n)
            fields.append((m2.group(1), typ.strip(), int(m2.group(2))) if m2 else (n, typ.strip(), 1))
    return fields


def _layout(fields):
    """offsets under the C rules for int (4) and pointers (8)"""
    off, out, align = 0, {}, 1
    for name, typ, n in fields:
        size = 8 if "*" in typ else 4
        assert typ in ("int", "const void*"), typ
        off = (off + size - 1) // size * size
        out[name] = off
        off += size * n
        align = max(align, size)
    return out, (off + align - 1) // align * align


def test_ctypes_mirrors_equal_the_header():
    from litepi._ffi import LpSurface, LpSurfaceFormat
    for cls, name, size in ((LpSurface, "lp_surface", 48), (LpSurfaceFormat, "lp_surface_format", 32)):
        offsets, total = _layout(_header_struct(name))
        assert total == size == C.sizeof(cls), (name, total, C.sizeof(cls))
        assert [f[0] for f in cls._fields_] == list(offsets), name
        for f in cls._fields_:
            assert getattr(cls, f[0]).offset == offsets[f[0]], (name, f[0])
    assert LpSurface.plane.offset == 0 and LpSurface.pitch.offset == 16 and LpSurface.height.offset == 24
    assert LpSurface.width.offset == 28 and LpSurface.reserved.offset == 32
    assert LpSurfaceFormat.pixfmt.offset == 0 and LpSurfaceFormat.matrix.offset == 4 and LpSurfaceFormat.reserved.offset == 8
    text = open(HEADER).read()
    assert re.search(r"enum lp_surface_pixfmt \{ LP_SURF_NV12 = 1, LP_SURF_P010 = 2 \}", text)
    from litepi import _ffi
    assert (_ffi.LP_SURF_NV12, _ffi.LP_SURF_P010) == (1, 2)
    assert "#define LP_ABI_VERSION 310" in text and _ffi.ABI_VERSION == 310


def test_new_symbols_are_exported():
    from litepi import _ffi
    lib = _ffi.load_library()
    text = open(HEADER).read()
    for s in ("lp_surfaces_check", "lp_run_surfaces_device", "lp_run_views_surfaces_device", "lp_test_convert_surfaces", "lp_graph_stats"):
        assert s in _ffi.SYMBOLS and hasattr(lib, s) and getattr(lib, s).restype is C.c_int
        assert re.search(r"\bint " + s + r"\(", text), s
    assert lib.lp_graph_stats(None, None, None, None, None) == _ffi.LP_ERR_ARG   # no handle: refused on the host


# ---------------------------------------------------------------------------- the Python helpers
def test_python_helpers_raise_before_any_handle():
    from litepi._ffi import LP_ERR_ARG, LitepiError
    from litepi.surfaces import Surface, surface_array, surface_format, surface_from_tensors, surfaces_check
    good = Surface(A, A + 4096, 4, 6)
    surfaces_check([good])
    surfaces_check([good, Surface(A, A + 4096, 720, 1280, 1280, 2048)], "nv12", "bt709")
    surfaces_check([Surface(A, A + 4096, 4, 6, 12, 14)], "p010")
    for bad in ([Surface(A, A + 4096, 5, 6)], [Surface(A, A + 4096, 4, 6, 5, 0)], [Surface(0, A, 4, 6)], [Surface(A, A, 4, 6, 0, -1)]):
        with pytest.raises(LitepiError) as ei:
            surfaces_check(bad)
        assert ei.value.code == LP_ERR_ARG
    with pytest.raises(LitepiError) as ei:
        surfaces_check([Surface(A + 1, A + 4096, 4, 6)], "p010")
    assert ei.value.code == LP_ERR_ARG
    for kw in (dict(pixfmt="p016"), dict(pixfmt="bgr"), dict(matrix="bt2020")):
        with pytest.raises(ValueError):
            surface_format(**kw)
        with pytest.raises(ValueError):
            surfaces_check([good], **kw)
    with pytest.raises(ValueError):
        surfaces_check([])
    with pytest.raises(ValueError):
        surface_array([(A, A, 4, 6)])
    for args in ((A, A, 4.5, 6), (A, A, 4, 6, 1 << 31, 0), (-1, A, 4, 6), (A, 1 << 64, 4, 6), (A, A, True, 6)):
        with pytest.raises(ValueError):
            Surface(*args)
    arr = surface_array([Surface(A, A + 8, 4, 6, 8, 10)])
    assert (arr[0].plane[0], arr[0].plane[1], arr[0].pitch[0], arr[0].pitch[1], arr[0].height, arr[0].width) == (A, A + 8, 8, 10, 4, 6)
    assert list(arr[0].reserved) == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        surface_from_tensors(np.zeros((4, 6), np.uint8), np.zeros((2, 6), np.uint8))   # arrays are no device tensors


def test_surface_from_tensors_reads_address_pitch_and_dtype():
    torch = pytest.importorskip("torch")
    from litepi.surfaces import surface_from_tensors

    class Dev:   # what the helper reads of a device tensor, on a host tensor's layout (no device is touched)
        def __init__(self, t):
            self.t = t
            self.is_cuda, self.dtype, self.shape, self.device = True, t.dtype, t.shape, "cuda:0"
        def data_ptr(self): return self.t.data_ptr()              # noqa: E704
        def stride(self, i): return self.t.stride(i)               # noqa: E704
        def element_size(self): return self.t.element_size()       # noqa: E704
        def dim(self): return self.t.dim()                         # noqa: E704

    y, uv = torch.zeros(4, 16, dtype=torch.uint8)[:, :6], torch.zeros(2, 10, dtype=torch.uint8)[:, 2:8]
    s, fmt = surface_from_tensors(Dev(y), Dev(uv))
    assert fmt == "nv12" and (s.height, s.width, s.pitch_y, s.pitch_uv) == (4, 6, 16, 10)
    assert (s.y_ptr, s.uv_ptr) == (y.data_ptr(), uv.data_ptr()) and s.uv_ptr == uv.data_ptr()
    y16, uv16 = torch.zeros(4, 16, dtype=torch.int16)[:, :6], torch.zeros(2, 3, 2, dtype=torch.int16)
    s, fmt = surface_from_tensors(Dev(y16), Dev(uv16))
    assert fmt == "p010" and (s.height, s.width, s.pitch_y, s.pitch_uv) == (4, 6, 32, 12)
    with pytest.raises(ValueError):   # host tensors are no surfaces
        surface_from_tensors(y, uv)
    with pytest.raises(ValueError):   # one sample type per surface
        surface_from_tensors(Dev(y), Dev(uv16))
    with pytest.raises(ValueError):
        surface_from_tensors(Dev(torch.zeros(4, 6)), Dev(torch.zeros(2, 6)))   # float planes
    with pytest.raises(ValueError):
        surface_from_tensors(Dev(y), Dev(torch.zeros(2, 8, dtype=torch.uint8)))   # chroma of another width
    with pytest.raises(ValueError):
        surface_from_tensors(Dev(torch.zeros(4, 12, dtype=torch.uint8)[:, ::2]), Dev(uv))   # samples not contiguous in a row


# ---------------------------------------------------------------------------- the helpers of the oracle
def test_narrowing_a_widened_frame_gives_it_back_whatever_the_low_bytes():
    rng = np.random.default_rng(11)
    frame = rng.integers(0, 256, (9, 10), dtype=np.uint8)
    frame[0, :4] = [0, 255, 16, 235]
    for wide in (S.widen(frame), S.widen(frame, low=0xFF), S.widen(frame, low=0xC0), S.widen(frame, rng=rng)):
        assert wide.dtype == np.uint16 and np.array_equal(S.narrow(wide), frame)
    assert int(S.widen(frame, low=0xFF)[0, 1]) == 0xFFFF and int(S.widen(frame)[0, 2]) == 0x1000
    wide = S.widen(frame, rng=rng)
    assert len(np.unique(wide & 0xFF)) > 16   # the low bytes are not all alike
    assert np.array_equal(S.surface_bgr(wide, "p010", "bt709"), S.surface_bgr(frame, "nv12", "bt709"))
    assert wide.tobytes()[1::2] == frame.tobytes()   # little-endian: the high byte is the second of each sample


def test_pack_plane_layout():
    rng = np.random.default_rng(12)
    rows = rng.integers(0, 256, (3, 5), dtype=np.uint8)
    buf, off = S.pack_plane(rows, pitch=8, offset=3, tail=2)
    assert off == 3 and buf.size == 3 + 2 * 8 + 5 + 2
    for r in range(3):
        assert np.array_equal(buf[3 + 8 * r:3 + 8 * r + 5], rows[r])
    mask = np.ones(buf.size, bool)
    for r in range(3):
        mask[3 + 8 * r:3 + 8 * r + 5] = False
    assert (buf[mask] == 0xEE).all()
    wide = S.widen(rows)
    buf, _ = S.pack_plane(wide, pitch=0, offset=2)
    assert buf.size == 2 + 3 * 10 and np.array_equal(buf[2:].view(np.uint16).reshape(3, 5), wide)
    y, uv = S.split_planes(np.zeros((9, 10), np.uint8))
    assert y.shape == (6, 10) and uv.shape == (3, 10)
