"""CPU tests of the pixel-format front door: the conversion oracle (tests/pixfmt_ref.py), lp_frame_layout (pure host, like
lp_tile_grid), the exported symbols, the host-frame shape checks of the Python backend and the --raw_frames reader.  No device."""
import ctypes as C

import numpy as np
import pytest

import pixfmt_ref as R


# ---------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_oracle_worked_cases(matrix):
    for (y, u, v), bgr in R.WORKED[matrix]:
        got = R.yuv_to_bgr(y, u, v, matrix)
        assert tuple(int(c) for c in got) == bgr, f"{matrix} {(y, u, v)}: {tuple(got)} vs {bgr}"


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_oracle_is_int32_safe(matrix):
    # every intermediate over all 2^24 inputs: luma terms depend on Y alone, chroma terms on (U, V) alone, so the extremes
    # of every sum are met on the 256 x 65536 grid evaluated as [256, 1, 1] x [1, 256, 256]
    Y = np.arange(256).reshape(256, 1, 1)
    U = np.arange(256).reshape(1, 256, 1)
    V = np.arange(256).reshape(1, 1, 256)
    lo = hi = 0
    for y0 in range(0, 256, 32):
        _, terms = R.yuv_to_bgr(Y[y0:y0 + 32], U, V, matrix, return_terms=True)
        lo = min([lo] + [int(t.min()) for t in terms])
        hi = max([hi] + [int(t.max()) for t in terms])
    assert -2**31 <= lo and hi < 2**31
    assert -2.9e8 <= lo and hi <= 5.8e8, (lo, hi)


def test_all_yuv_frames_hold_every_combination_once():
    seen = np.zeros(1 << 24, np.uint8)
    for f in R.all_yuv_frames():
        assert f.shape == (768, 512) and f.dtype == np.uint8
        Y = f[:512].astype(np.int64)
        uv = f[512:].reshape(256, 256, 2).astype(np.int64)
        U = np.repeat(np.repeat(uv[..., 0], 2, 0), 2, 1)
        V = np.repeat(np.repeat(uv[..., 1], 2, 0), 2, 1)
        np.add.at(seen, ((Y << 16) | (U << 8) | V).ravel(), 1)
    assert int(seen.min()) == 1 and int(seen.max()) == 1


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_product_host_conversion_equals_oracle(matrix):
    # litepi/pixfmt.py draws the --save_viz overlays; it restates the formula in int32 and must agree with the int64 oracle
    from litepi.pixfmt import nv12_to_bgr
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (18 * 3 // 2, 22), dtype=np.uint8)
    frame[:2, :4] = [[0, 255, 16, 235], [0, 255, 16, 235]]
    frame[18, :4] = [0, 0, 255, 255]
    assert np.array_equal(nv12_to_bgr(frame, matrix), R.nv12_to_bgr(frame, matrix))


def test_forward_helper_round_trip_is_close():
    # bgr_to_nv12 only builds inputs; still, smooth content must survive the round trip to within the chroma subsampling
    yy, xx = np.mgrid[0:32, 0:48]
    img = np.stack([xx * 5, yy * 7, 255 - xx * 3 - yy * 2], -1).clip(0, 255).astype(np.uint8)
    back = R.nv12_to_bgr(R.bgr_to_nv12(img), "bt601")
    assert np.abs(back.astype(int) - img.astype(int)).max() <= 12


def test_pack_frames_layout():
    rng = np.random.default_rng(4)
    frames = [rng.integers(0, 256, (9, 10), dtype=np.uint8) for _ in range(2)]   # 6 x 10
    buf, uv, fb, st = R.pack_frames(frames, pitch=12, uv_offset=80, frame_stride=130)
    assert (uv, fb, st) == (80, 80 + 36, 130) and buf.size == 130 + 116
    assert np.array_equal(buf[130 + 12 * 5:130 + 12 * 5 + 10], frames[1][5])
    assert np.array_equal(buf[80 + 24:80 + 34], frames[0][8])
    assert buf[10] == 0xEE and buf[72] == 0xEE and buf[120] == 0xEE


# ---------------------------------------------------------------------------- the library, host only
@pytest.fixture(scope="module")
def lib():
    from litepi import _ffi
    return _ffi.load_library()


def _fmt(**kw):
    from litepi._ffi import LpFrameFormat
    f = LpFrameFormat()
    f.pixfmt = 1
    for k, v in kw.items():
        if k == "reserved":
            f.reserved[v] = 1
        else:
            setattr(f, k, v)
    return f


def _layout(lib, f, H, W):
    uv, nb = C.c_int64(-1), C.c_int64(-1)
    rc = lib.lp_frame_layout(C.byref(f) if f is not None else None, H, W, C.byref(uv), C.byref(nb))
    return rc, uv.value, nb.value


def test_library_exports_the_new_symbols(lib):
    from litepi import _ffi
    for s in ("lp_frame_layout", "lp_set_input_format", "lp_test_convert_frames"):
        assert s in _ffi.SYMBOLS
        assert getattr(lib, s) is not None
    assert lib.lp_version() == 310
    assert C.sizeof(_ffi.LpFrameFormat) == 56


def test_frame_layout_resolves_zeros(lib):
    assert _layout(lib, _fmt(), 640, 640) == (0, 409600, 614400)
    assert _layout(lib, _fmt(matrix=1), 720, 1280) == (0, 921600, 1382400)
    assert _layout(lib, _fmt(pitch=1280), 682, 1198) == (0, 1280 * 682, 1280 * 682 + 1280 * 341)
    assert _layout(lib, _fmt(pitch=1280, uv_offset=1280 * 688), 682, 1198) == (0, 1280 * 688, 1280 * 688 + 1280 * 341)
    assert _layout(lib, _fmt(frame_stride=1 << 20), 640, 640) == (0, 409600, 614400)
    assert _layout(lib, _fmt(), 2, 2) == (0, 4, 6)
    # packed BGR: by a NULL format and by LP_PIX_BGR8
    assert _layout(lib, None, 5, 7) == (0, 0, 105)
    assert _layout(lib, _fmt(pixfmt=0), 5, 7) == (0, 0, 105)
    # the outputs may be NULL
    assert lib.lp_frame_layout(C.byref(_fmt()), 640, 640, None, None) == 0
    from litepi.backend import frame_layout
    assert frame_layout(640, 640) == (409600, 614400)
    assert frame_layout(682, 1198, pitch=1280) == (1280 * 682, 1280 * 1023)


@pytest.mark.parametrize("case,f,H,W", [
    ("odd H", dict(), 641, 640), ("odd W", dict(), 640, 639), ("pitch < W", dict(pitch=638), 640, 640),
    ("uv_offset < pitch*H", dict(uv_offset=409599), 640, 640), ("uv_offset < pitch*H (pitched)", dict(pitch=704, uv_offset=409600), 640, 640),
    ("frame_stride < frame", dict(frame_stride=614399), 640, 640),
    ("unknown pixfmt", dict(pixfmt=2), 640, 640), ("negative pixfmt", dict(pixfmt=-1), 640, 640),
    ("unknown matrix", dict(matrix=2), 640, 640), ("reserved0", dict(reserved0=1), 640, 640),
    ("reserved[0]", dict(reserved=0), 640, 640), ("reserved[5]", dict(reserved=5), 640, 640),
    ("BGR with a pitch", dict(pixfmt=0, pitch=1920), 640, 640), ("BGR with a uv_offset", dict(pixfmt=0, uv_offset=8), 640, 640),
    ("BGR with a frame_stride", dict(pixfmt=0, frame_stride=1 << 21), 640, 640),
    ("negative pitch", dict(pitch=-640), 640, 640), ("empty frame", dict(), 0, 640),
])
def test_frame_layout_rejects(lib, case, f, H, W):
    from litepi._ffi import LP_ERR_ARG
    rc, _, _ = _layout(lib, _fmt(**f), H, W)
    assert rc == LP_ERR_ARG, case
    assert len(lib.lp_last_error()) > 0
    assert _layout(lib, _fmt(), 640, 640)[0] == 0   # and a good call right after


def test_frame_layout_python_raises(lib):
    from litepi._ffi import LP_ERR_ARG, LitepiError
    from litepi.backend import frame_layout
    with pytest.raises(LitepiError) as ex:
        frame_layout(641, 640)
    assert ex.value.code == LP_ERR_ARG
    with pytest.raises(ValueError):
        frame_layout(640, 640, pixfmt="i420")
    with pytest.raises(ValueError):
        frame_layout(640, 640, matrix="bt2020")


# ---------------------------------------------------------------------------- host-frame shape checks (no handle is created)
def _bare_engine(pixel_format):
    from litepi import Engine
    e = Engine.__new__(Engine)
    e._h = None
    e.pixel_format, e.csc_matrix, e._tight_frames = pixel_format, "bt601", True
    return e


def test_img_args_nv12_shapes():
    e = _bare_engine("nv12")
    frames = [np.zeros((960, 640), np.uint8), np.zeros((1080, 1280), np.uint8), np.zeros((3, 2), np.uint8)]
    imgs, ptrs, hs, ws = e._img_args(frames, frames=True)
    assert list(hs) == [640, 720, 2] and list(ws) == [640, 1280, 2]
    assert [p for p in ptrs] == [i.ctypes.data for i in imgs]
    assert e.frame_hw(frames[1]) == (720, 1280)
    for bad in (np.zeros((640, 640, 3), np.uint8),      # a BGR image is not silently taken for NV12
                np.zeros((961, 640), np.uint8),         # rows not a multiple of 3
                np.zeros((960, 641), np.uint8),         # odd width
                np.zeros((960,), np.uint8), np.zeros((0, 640), np.uint8)):
        with pytest.raises(ValueError):
            e._img_args([bad], frames=True)
    # crops for the classifier and the test hooks stay BGR whatever the frame format is
    _, _, hs, ws = e._img_args([np.zeros((5, 7, 3), np.uint8)])
    assert list(hs) == [5] and list(ws) == [7]
    e._tight_frames = False
    with pytest.raises(ValueError):
        e._img_args(frames[:1], frames=True)


def test_img_args_bgr_unchanged():
    e = _bare_engine("bgr")
    _, _, hs, ws = e._img_args([np.zeros((5, 7, 3), np.uint8)], frames=True)
    assert list(hs) == [5] and list(ws) == [7]
    assert e.frame_hw(np.zeros((5, 7, 3), np.uint8)) == (5, 7)
    with pytest.raises(ValueError):
        e._img_args([np.zeros((960, 640), np.uint8)], frames=True)


# ---------------------------------------------------------------------------- the --raw_frames reader
def test_raw_frames_reader(tmp_path):
    from litepi import e2e
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (3, 12, 10), dtype=np.uint8)   # three 10 x 8 NV12 frames
    p = tmp_path / "clip.nv12"
    frames.tofile(p)
    got = e2e.read_raw_frames(p, 10, 8, "nv12")
    assert got.shape == (3, 12, 10) and np.array_equal(np.asarray(got), frames)
    bgr = rng.integers(0, 256, (2, 8, 10, 3), dtype=np.uint8)
    q = tmp_path / "clip.bgr"
    bgr.tofile(q)
    got = e2e.read_raw_frames(q, 10, 8, "bgr")
    assert got.shape == (2, 8, 10, 3) and np.array_equal(np.asarray(got), bgr)
    with open(p, "ab") as f:   # a trailing partial frame
        f.write(b"\x00" * 7)
    with pytest.raises(ValueError, match="whole number"):
        e2e.read_raw_frames(p, 10, 8, "nv12")
    (tmp_path / "empty.nv12").write_bytes(b"")
    with pytest.raises(ValueError):
        e2e.read_raw_frames(tmp_path / "empty.nv12", 10, 8, "nv12")
    with pytest.raises(ValueError):
        e2e.read_raw_frames(q, 9, 8, "nv12")
    assert e2e.parse_frame_size("1280x720") == (1280, 720)
    for bad in ("1280", "axb", "0x720", None):
        with pytest.raises(ValueError):
            e2e.parse_frame_size(bad)
    names = [e2e.RawFrame(i, tmp_path).name for i in (0, 1, 41)]
    assert names == ["frame_000001", "frame_000002", "frame_000042"]


def test_cli_flags_and_refusals(tmp_path):
    from litepi import e2e
    clip = str(tmp_path / "clip.nv12")
    np.zeros((2, 12, 10), np.uint8).tofile(clip)
    a = e2e.build_parser().parse_args(["--raw_frames", clip, "--frame_size", "10x8", "--pixel_format", "nv12", "--csc_matrix", "bt709"])
    assert (a.raw_frames, a.frame_size, a.pixel_format, a.csc_matrix) == (clip, "10x8", "nv12", "bt709")
    e2e.check_frame_args(a)
    with pytest.raises(ValueError, match="whole number"):   # 240 bytes are not a whole number of 12 x 8 frames
        e2e.check_frame_args(e2e.build_parser().parse_args(["--raw_frames", clip, "--frame_size", "12x8", "--pixel_format", "nv12"]))
    d = e2e.build_parser().parse_args([])
    assert (d.raw_frames, d.pixel_format, d.csc_matrix) == (None, "bgr", "bt601")
    e2e.check_frame_args(d)
    with pytest.raises(SystemExit):   # nv12 describes raw frames: images are decoded to BGR
        e2e.check_frame_args(e2e.build_parser().parse_args(["--pixel_format", "nv12"]))
    with pytest.raises(SystemExit):
        e2e.check_frame_args(e2e.build_parser().parse_args(["--raw_frames", clip]))
