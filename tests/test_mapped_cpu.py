"""Mapped views without a GPU (include/litepi.h "mapped views"):

1. lp_map_fixed, lp_map_render and lp_map_box on the loaded library == tests/mapped_ref.py's NumPy restatement of the three
   rules, bit for bit, on integer crops, a half-pixel shifted crop, a 7 degree rotation at scale 1.3, a barrel map, a map
   wholly outside the frame, uniformly random positions and maps whose taps include the frame's last pixel;
2. their error codes; the new symbols, the unchanged ABI version;
3. tests/native/map_rule_check.cpp: csrc/view_map.h alone under -fsanitize=address,undefined against heap frames of exactly
   H * W * 3 bytes;
4. litepi/lens.py's builders; the ValueErrors of HybridPipeline(view_maps=...) and the CLI's --view_maps checks.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mapped_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 64
FRAMES = [(150, 210), (70, 720)]
CASE_NAMES = list(M.cases(S, *FRAMES[0]))


def _frame(hw):
    return np.random.default_rng(hw[0] * 31 + hw[1]).integers(0, 256, hw + (3,), dtype=np.uint8)


@pytest.fixture(scope="module")
def lib():
    from litepi import _ffi
    return _ffi.load_library()


# ---------------------------------------------------------------------------- 1. the three rules, bit for bit
@pytest.mark.parametrize("hw", FRAMES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("name", CASE_NAMES)
def test_map_rules_equal_numpy_bit_for_bit(lib, hw, name):
    from litepi import backend
    H, W = hw
    xy = M.cases(S, H, W)[name]
    want_fx = M.fixed(xy, H, W)
    fx = backend.map_fixed(xy, H, W)
    assert fx.dtype == np.int32 and np.array_equal(fx, want_fx), f"{name}: {int((fx != want_fx).sum())} table entries differ"
    if name == "half_pixel":
        assert np.all(fx & 31 == 16)
    if name == "outside":
        assert np.all(fx[..., 0] == (W + 1) * 32) and np.all(fx[..., 1] == (H + 1) * 32)
    if name.startswith("last_pixel"):   # the last view pixel's taps end on (or start at) the frame's last pixel
        ix, iy = fx[-1, -1] >> 5
        ax, ay = fx[-1, -1] & 31
        assert (ix + (1 if ax else 0), iy + (1 if ay else 0)) == (W - 1, H - 1) and (bool(ax), bool(ay)) == (name.endswith("frac"),) * 2
    frame = _frame(hw)
    want = M.render(want_fx, frame)
    got = backend.map_render(fx, frame)
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} bytes differ, first at {np.argwhere(got != want)[0].tolist()}"
    if name == "crop":
        assert np.array_equal(got, frame[3:3 + S, 17:17 + S]), "an integer crop map is the crop"
    if name == "outside":
        assert np.all(got == 114)
    b = M.boxes(S, seed=H + W)
    want_b = M.map_box(want_fx, H, W, b)
    got_b = backend.map_box(fx, H, W, b)
    bad = np.argwhere(got_b.view(np.uint32) != want_b.view(np.uint32))
    assert bad.size == 0, f"{name}: {len(bad)} coordinates differ, first box {b[bad[0][0]]}: {got_b[bad[0][0]]} vs {want_b[bad[0][0]]}"
    assert np.all(got_b[:, 0] <= got_b[:, 2]) and np.all(got_b[:, 1] <= got_b[:, 3])
    assert got_b.min() >= 0 and got_b[:, [0, 2]].max() <= W and got_b[:, [1, 3]].max() <= H
    if name == "crop":   # an integer crop map moves a box by the crop's origin
        inner = b[(b[:, 0] > 1) & (b[:, 1] > 1) & (b[:, 2] < S - 1) & (b[:, 3] < S - 1)]
        assert np.allclose(backend.map_box(fx, H, W, inner), inner + np.float32([17, 3, 17, 3]), atol=1e-4, rtol=0)


def test_map_fixed_rounds_half_to_even_and_clamps(lib):
    from litepi import backend
    xy = np.zeros((S, S, 2), np.float32)
    vals = np.float32([0.015625, 0.046875, -0.015625, -5.0, 1e9, -np.inf, np.inf, 209.984375, 3.0 + 1 / 64, 211.0, 211.5])
    xy[0, :len(vals), 0] = vals
    fx = backend.map_fixed(xy, 150, 210)[0, :len(vals), 0]
    assert fx.tolist() == [0, 2, 0, -64, 211 * 32, -64, 211 * 32, 6720, 96, 211 * 32, 211 * 32]


# ---------------------------------------------------------------------------- 2. error codes, symbols
def test_map_host_functions_error_codes(lib):
    from litepi import _ffi
    fp = C.POINTER(C.c_float)
    xy = M.crop(S, 3, 4)
    fx = np.zeros((S, S, 2), np.int32)
    frame = _frame((20, 30))
    out = np.zeros((S, S, 3), np.uint8)
    box, obox = np.float32([1, 2, 3, 4]), np.zeros(4, np.float32)
    xp, bp, op = xy.ctypes.data_as(fp), box.ctypes.data_as(fp), obox.ctypes.data_as(fp)
    assert lib.lp_map_fixed(xp, S, 20, 30, fx.ctypes.data) == _ffi.LP_OK
    assert lib.lp_map_render(fx.ctypes.data, S, frame.ctypes.data, 20, 30, out.ctypes.data) == _ffi.LP_OK
    assert lib.lp_map_box(fx.ctypes.data, S, 20, 30, bp, op) == _ffi.LP_OK
    for bad in ((None, S, 20, 30, fx.ctypes.data), (xp, S, 20, 30, None), (xp, 1, 20, 30, fx.ctypes.data), (xp, 0, 20, 30, fx.ctypes.data),
                (xp, 16385, 20, 30, fx.ctypes.data), (xp, S, 0, 30, fx.ctypes.data), (xp, S, 20, -1, fx.ctypes.data),
                (xp, S, 16385, 30, fx.ctypes.data), (xp, S, 20, 16385, fx.ctypes.data)):
        assert lib.lp_map_fixed(*bad) == _ffi.LP_ERR_ARG, bad[1:4]
    for where in ((0, 0, 0), (S - 1, S - 1, 1), (17, 5, 0)):
        nan = xy.copy()
        nan[where] = np.nan
        assert lib.lp_map_fixed(nan.ctypes.data_as(fp), S, 20, 30, fx.ctypes.data) == _ffi.LP_ERR_ARG
        assert b"NaN" in lib.lp_last_error()
    for bad in ((None, S, frame.ctypes.data, 20, 30, out.ctypes.data), (fx.ctypes.data, S, None, 20, 30, out.ctypes.data),
                (fx.ctypes.data, S, frame.ctypes.data, 20, 30, None), (fx.ctypes.data, 1, frame.ctypes.data, 20, 30, out.ctypes.data),
                (fx.ctypes.data, S, frame.ctypes.data, 0, 30, out.ctypes.data), (fx.ctypes.data, S, frame.ctypes.data, 20, 16385, out.ctypes.data)):
        assert lib.lp_map_render(*bad) == _ffi.LP_ERR_ARG
    for bad in ((None, S, 20, 30, bp, op), (fx.ctypes.data, S, 20, 30, None, op), (fx.ctypes.data, S, 20, 30, bp, None),
                (fx.ctypes.data, 1, 20, 30, bp, op), (fx.ctypes.data, S, 0, 30, bp, op), (fx.ctypes.data, S, 20, 0, bp, op)):
        assert lib.lp_map_box(*bad) == _ffi.LP_ERR_ARG
    assert lib.lp_map_add(None, xp, 20, 30, C.byref(C.c_int())) == _ffi.LP_ERR_ARG
    assert lib.lp_map_clear(None) == _ffi.LP_ERR_ARG


def test_map_symbols_and_abi(lib):
    from litepi import _ffi
    for s in ("lp_map_fixed", "lp_map_render", "lp_map_box", "lp_map_add", "lp_map_clear", "lp_run_mapped", "lp_run_mapped_device",
              "lp_test_map_views", "lp_test_map_boxes"):
        assert s in _ffi.SYMBOLS and hasattr(lib, s)
    assert lib.lp_version() == 310 == _ffi.ABI_VERSION and _ffi.LP_MAP_MAX == 64
    header = open(os.path.join(ROOT, "include", "litepi.h")).read()
    assert "#define LP_MAP_MAX 64" in header and "NOT cv2.remap's weight table" in header
    rule = open(os.path.join(ROOT, "yolo-litepi_amd", "csrc", "view_map.h")).read()
    assert "not cv2.remap's weight table" in rule


# ---------------------------------------------------------------------------- 3. the header under sanitizers
def test_view_map_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "map_rule_check")
    src = os.path.join(ROOT, "tests", "native", "map_rule_check.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", inc, src, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK" and lines[-2] == "frames 8 fails 0", lines[-2:]


# ---------------------------------------------------------------------------- 4. lens.py
def _K(f, cx, cy):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], dtype=np.float64)


@pytest.mark.parametrize("scale", [1.0, 0.75])
def test_lens_pinholes_without_distortion_are_crop_maps(scale):
    """zero distortion, zero rotation and a matching field of view: the view is a crop at `scale` frame pixels per view pixel.
    The positions are multiples of 1/8, far from a float32 rounding boundary, so both casts land on the same float."""
    from litepi import lens
    hfov = 70.0
    f_view = (S / 2.0) / np.tan(np.radians(hfov) / 2.0)
    cx, cy = 300.5, 200.5
    K = _K(f_view * scale, cx, cy)
    want = lens.crop_map(S, cx + 0.5 - scale * S / 2.0, cy + 0.5 - scale * S / 2.0, scale)
    for got in (lens.pinhole_from_brown(S, K, (0, 0, 0, 0, 0), hfov=hfov), lens.pinhole_from_brown(S, K, (), hfov=hfov)):
        assert got.dtype == np.float32 and got.shape == (S, S, 2)
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 1e-6
    assert np.array_equal(want, M.crop(S, cx + 0.5 - scale * S / 2.0, cy + 0.5 - scale * S / 2.0, scale))


def test_lens_centre_ray_lands_on_the_principal_point():
    """an odd view side has a centre pixel: its ray is the view axis, which every lens model sends to (cx, cy) when the view is
    not turned -- whatever the distortion; turned by a yaw, the fisheye's centre ray lands f * yaw right of it (equidistant)"""
    from litepi import lens
    n, c = 65, 32
    K = _K(410.0, 333.25, 207.5)
    for xy in (lens.pinhole_from_brown(n, K, (-0.3, 0.1, 0.001, -0.002, 0.01), hfov=100.0, roll=33.0),
               lens.pinhole_from_fisheye(n, K, (0.05, -0.01, 0.002, 0.0), hfov=120.0, roll=-12.0)):
        assert np.abs(xy[c, c].astype(np.float64) - [333.25, 207.5]).max() <= 1e-4
    xy = lens.pinhole_from_fisheye(n, K, (), yaw=40.0, hfov=90.0)
    assert np.abs(xy[c, c].astype(np.float64) - [333.25 + 410.0 * np.radians(40.0), 207.5]).max() <= 1e-3
    pano = lens.pinhole_from_equirect(n, 512, 1024, hfov=90.0)
    assert np.abs(pano[c, c].astype(np.float64) - [511.5, 255.5]).max() <= 1e-4
    # a pinhole lens cannot show what lies behind it: those pixels are outside every frame
    back = lens.pinhole_from_brown(n, K, (), yaw=180.0, hfov=90.0)
    assert np.all(back == lens.OUTSIDE)


def test_lens_equirect_yaw_is_a_column_shift():
    """a yaw of 90 degrees moves every view pixel W / 4 columns to the right in the panorama (modulo its width); float32 casts of
    positions below 1024 differ by at most one ulp of 6.1e-5 each"""
    from litepi import lens
    H, W = 512, 1024
    for pitch, roll in ((0.0, 0.0), (20.0, 15.0)):
        a = lens.pinhole_from_equirect(S, H, W, yaw=0.0, pitch=pitch, roll=roll, hfov=80.0).astype(np.float64)
        b = lens.pinhole_from_equirect(S, H, W, yaw=90.0, pitch=pitch, roll=roll, hfov=80.0).astype(np.float64)
        dx = np.mod(b[..., 0] - a[..., 0] - W / 4.0 + W / 2.0, W) - W / 2.0
        assert np.abs(dx).max() <= 2e-4 and np.abs(b[..., 1] - a[..., 1]).max() <= 2e-4
    assert a[..., 0].min() >= -0.5 and b[..., 0].max() < W - 0.5 + 1e-3


def test_lens_builders_reject_bad_arguments():
    from litepi import lens
    K = _K(100.0, 50.0, 50.0)
    with pytest.raises(ValueError):
        lens.pinhole_from_brown(S, K, (), hfov=180.0)
    with pytest.raises(ValueError):
        lens.pinhole_from_brown(S, np.eye(2), ())
    with pytest.raises(ValueError):
        lens.pinhole_from_brown(S, K, (0,) * 6)
    with pytest.raises(ValueError):
        lens.pinhole_from_fisheye(S, K, (0,) * 5)


# ---------------------------------------------------------------------------- 5. pipeline and CLI argument checks
def test_pipeline_view_maps_value_errors():
    """every one of these is raised before a handle exists (no GPU here: creating one would fail otherwise)"""
    from litepi import HybridPipeline
    maps = [M.crop(320, 0, 0)]
    base = dict(detector_param="none.param", detector_bin="none.bin", classifier_path="none.pth", classifier_arch="shufflenetv2",
                num_classes=4, max_batch=4)
    bad = [dict(det_input_size=(192, 320), view_maps=maps, view_maps_frame=(400, 500)),                       # rectangular
           dict(det_input_size=320, view_maps=maps, view_maps_frame=(400, 500), focus=1, track=True),          # focus
           dict(det_input_size=320, view_maps=maps, view_maps_frame=(400, 500), tile_overlap=64),              # tile_overlap
           dict(det_input_size=320, view_maps=maps, view_maps_frame=(400, 500), view_tile=480),
           dict(det_input_size=320, view_maps=maps),                                                           # no frame size
           dict(det_input_size=320, view_maps_frame=(400, 500)),                                               # no maps
           dict(det_input_size=320, view_maps=[], view_maps_frame=(400, 500)),
           dict(det_input_size=320, view_maps=[M.crop(64, 0, 0)], view_maps_frame=(400, 500)),                 # a map of another S
           dict(det_input_size=320, view_maps=[np.zeros((320, 320, 3), np.float32)], view_maps_frame=(400, 500)),
           dict(det_input_size=320, view_maps=[np.full((320, 320, 2), np.nan, np.float32)], view_maps_frame=(400, 500)),
           dict(det_input_size=320, view_maps=maps * 65, view_maps_frame=(400, 500))]
    for kw in bad:
        with pytest.raises(ValueError):
            HybridPipeline(**base, **kw)


def test_cli_view_maps_checks(tmp_path):
    from litepi import e2e
    good = str(tmp_path / "maps.npz")
    np.savez(good, xy=np.stack([M.crop(320, 0, 0), M.crop(320, 5, 6)]), frame=np.int64([400, 500]))
    xy, frame = e2e.load_view_maps(good, 320)
    assert xy.shape == (2, 320, 320, 2) and xy.dtype == np.float32 and frame == (400, 500)
    assert e2e.load_view_maps(good, (320, 320))[1] == (400, 500)

    p = e2e.build_parser()
    assert p.parse_args([]).view_maps is None
    base = ["--det_input_size", "320", "--view_maps", good]
    e2e.check_frame_args(p.parse_args(base))
    e2e.check_frame_args(p.parse_args(base + ["--views", "full;0,0,100,100", "--view_merge", "union"]))
    for bad in (base + ["--tile_overlap", "64"], base + ["--view_tile", "480"], base + ["--focus", "2", "--track"],
                ["--det_input_size", "192x320", "--view_maps", good], ["--det_input_size", "640", "--view_maps", good],
                ["--det_input_size", "320", "--view_maps", str(tmp_path / "absent.npz")]):
        with pytest.raises(SystemExit):
            e2e.check_frame_args(p.parse_args(bad))
    for name, content in (("nokey", dict(xy=xy)), ("shape", dict(xy=xy[0], frame=np.int64([400, 500]))),
                          ("frame", dict(xy=xy, frame=np.int64([400]))), ("nan", dict(xy=xy * np.float32(np.nan), frame=np.int64([400, 500])))):
        path = str(tmp_path / (name + ".npz"))
        np.savez(path, **content)
        with pytest.raises(SystemExit):
            e2e.load_view_maps(path, 320)
