"""Scaled views on the CPU: the library's pure-host entry points (lp_view_grid, lp_view_geometry) against the Python rule of
tests/views_ref.py, their argument errors, and the merge oracle on a sign seen at two scales."""
import ctypes as C

import numpy as np
import pytest

import tiling_ref as T
import views_ref as V


@pytest.mark.parametrize("H,W,tile,overlap,xs,ys,side", [
    (2048, 2048, 1280, 256, [0, 768], [0, 768], (1280, 1280)),          # 4 windows + full
    (1080, 1920, 960, 0, [0, 960], [0, 120], (960, 960)),
    (1080, 1920, 1280, 320, [0, 640], [0], (1280, 1080)),                # L <= tile on one axis: a window of side L
    (2048, 2048, 640, 128, [0, 512, 1024, 1408], [0, 512, 1024, 1408], (640, 640)),
    (700, 900, 320, 64, [0, 256, 512, 580], [0, 256, 380], (320, 320)),
])
def test_view_grid_worked_cases(H, W, tile, overlap, xs, ys, side):
    from litepi.backend import view_grid   # the library's lp_view_grid (host only)
    assert V.view_axis(W, tile, overlap) == (xs, side[0]) and V.view_axis(H, tile, overlap) == (ys, side[1])
    views = V.view_grid(tile, H, W, overlap, True)
    assert views[0] == (-1, -1, W, H)
    assert views[1:] == [(x, y, side[0], side[1]) for y in ys for x in xs]
    assert view_grid(tile, H, W, overlap, True) == views
    assert view_grid(tile, H, W, overlap, False) == views[1:] == V.view_grid(tile, H, W, overlap, False)


def test_view_grid_2048_tile1280_is_5_views():
    from litepi.backend import view_grid
    assert len(view_grid(1280, 2048, 2048, 256, True)) == len(V.view_grid(1280, 2048, 2048, 256, True)) == 5


@pytest.mark.parametrize("full", [True, False])
def test_view_grid_frame_that_fits_one_window(full):
    from litepi.backend import view_grid
    for H, W, tile in [(640, 640, 640), (300, 500, 640), (1280, 1280, 1280), (16, 16, 16)]:
        assert view_grid(tile, H, W, 0, full) == V.view_grid(tile, H, W, 0, full) == [(-1, -1, W, H)]


@pytest.mark.parametrize("S", [640, 320])
@pytest.mark.parametrize("full", [True, False])
def test_view_grid_at_det_input_equals_tile_grid(S, full):
    from litepi.backend import tile_grid, view_grid
    for H, W in [(2048, 2048), (681, 1198), (2000, S), (S, S), (S + 1, S + 1), (1024, 1280)]:
        for ov in (0, 128, 170, 171, S - 1):
            assert view_grid(S, H, W, ov, full) == tile_grid(S, H, W, ov, full) == T.tile_grid(S, H, W, ov, full), (H, W, ov)


def test_view_grid_matches_python_on_random_cases():
    from litepi.backend import view_grid
    rng = np.random.default_rng(4)
    for _ in range(200):
        H, W = (int(v) for v in rng.integers(16, 3000, 2))
        tile = int(rng.integers(16, 2000))
        ov = int(rng.integers(0, tile))
        if len(V.view_grid(tile, H, W, ov, True)) > 4096:
            continue
        full = bool(rng.integers(0, 2))
        assert view_grid(tile, H, W, ov, full) == V.view_grid(tile, H, W, ov, full), (H, W, tile, ov, full)


def _lib_views(call):
    """a grid of the library as an int32 [n, 4] array: call(n, buf, cap) is lp_tile_grid / lp_view_grid with its leading arguments bound"""
    from litepi import _ffi
    n = C.c_int()
    assert call(C.byref(n), None, 0) == _ffi.LP_OK
    buf = np.empty((n.value, 4), np.int32)
    assert call(C.byref(n), buf.ctypes.data_as(C.POINTER(C.c_int)), n.value) == _ffi.LP_OK
    return buf


def _ref_views(grid, axis, side, H, W, full):
    """The reference's grid as an array.  Up to 4096 windows it is the reference's own list (tiling_ref.tile_grid,
    views_ref.view_grid); a longer one (up to four million windows at overlap = tile - 1) is put together here from the
    reference's axis rule, row-major behind the whole frame, without a Python tuple per window."""
    xs, ys = axis(W), axis(H)
    if len(xs) * len(ys) <= 4096:
        return np.array(grid(H, W, full), np.int32).reshape(-1, 4)
    v = np.empty((len(ys), len(xs), 4), np.int32)
    v[..., 0], v[..., 1] = np.array(xs, np.int32)[None, :], np.array(ys, np.int32)[:, None]
    v[..., 2], v[..., 3] = side(W), side(H)
    head = np.array([[-1, -1, W, H]], np.int32) if full else np.empty((0, 4), np.int32)
    return np.concatenate([head, v.reshape(-1, 4)])


@pytest.mark.parametrize("tile", [64, 320, 640])
def test_both_grids_equal_their_references_over_the_size_sweep(tile):
    """lp_tile_grid (det_input = tile) and lp_view_grid share one axis and one emitter in the library; the two differ in the
    window's side where the frame is not larger than the tile (the tile's against the frame's)."""
    from litepi import _ffi
    from litepi.backend import _tiling
    lib = _ffi.load_library()
    sizes = (16, 63, 64, 65, 320, 321, 640, 641, 1279, 2048)
    n_cases = n_differ = 0
    for ov in (0, 1, tile // 2, tile - 1):
        for full in (True, False):
            t = _tiling(ov, full)
            for H in sizes:
                for W in sizes:
                    tiles = _lib_views(lambda n, buf, cap: lib.lp_tile_grid(tile, C.byref(t), H, W, n, buf, cap))
                    views = _lib_views(lambda n, buf, cap: lib.lp_view_grid(tile, ov, int(full), H, W, n, buf, cap))
                    exp_t = _ref_views(lambda h, w, f: T.tile_grid(tile, h, w, ov, f), lambda L: T.tile_axis(L, tile, ov), lambda L: tile,
                                       H, W, full)
                    exp_v = _ref_views(lambda h, w, f: V.view_grid(tile, h, w, ov, f), lambda L: V.view_axis(L, tile, ov)[0],
                                       lambda L: V.view_axis(L, tile, ov)[1], H, W, full)
                    assert np.array_equal(tiles, exp_t), ("lp_tile_grid", tile, ov, full, H, W)
                    assert np.array_equal(views, exp_v), ("lp_view_grid", tile, ov, full, H, W)
                    n_cases += 1
                    n_differ += not np.array_equal(tiles, views)
    assert n_cases == 800 and n_differ > 0   # e.g. a 63 x 2048 frame at tile 64: crops of 64 x 64, windows of 63 x 64


def _geometry_bits(g):
    return (np.array([g["ratio"], g["pad_w"], g["pad_h"]], np.float32).view(np.uint32).tolist(),
            (g["new_w"], g["new_h"], g["top"], g["left"]))


def test_view_geometry_bit_for_bit():
    from litepi.backend import view_geometry
    rng = np.random.default_rng(9)
    n = 0
    for S in (640, 320, 64):
        for _ in range(18):
            H, W = (int(v) for v in rng.integers(16, 2500, 2))
            w, h = int(rng.integers(16, W + 1)), int(rng.integers(16, H + 1))
            x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
            for view in ((x, y, w, h), (-1, -1, W, H), (-1, 7, 3, 5), (0, 0, W, H)):
                assert _geometry_bits(view_geometry(S, H, W, view)) == _geometry_bits(V.view_geometry(S, H, W, view)), (S, H, W, view)
                n += 1
    assert n >= 50
    # the whole-frame view is the window {0, 0, W, H}, and both are the letterbox geometry of the frame
    from oracle import postprocess_ref as P
    r, (nw, nh), (dw, dh), (top, _, left, _) = P.letterbox_params(1080, 1920, 640)
    g = view_geometry(640, 1080, 1920, "full")
    assert _geometry_bits(g) == _geometry_bits(view_geometry(640, 1080, 1920, (0, 0, 1920, 1080)))
    assert _geometry_bits(g) == _geometry_bits(dict(ratio=np.float32(r), pad_w=np.float32(dw), pad_h=np.float32(dh), new_w=nw, new_h=nh,
                                                    top=top, left=left))
    # a native window is tiled inference's crop: ratio 1, pad = -(x, y)
    g = view_geometry(640, 2048, 2048, (512, 1408, 640, 640))
    assert (float(g["ratio"]), float(g["pad_w"]), float(g["pad_h"]), g["top"], g["left"]) == (1.0, -512.0, -1408.0, 0, 0)


def test_view_argument_errors():
    from litepi import _ffi
    lib = _ffi.load_library()
    n = C.c_int()
    ok = lambda *a: lib.lp_view_grid(*a)
    assert ok(640, 128, 1, 2048, 2048, C.byref(n), None, 0) == _ffi.LP_OK and n.value == 17
    for tile, ov, full in [(15, 0, 1), (640, -1, 1), (640, 640, 1), (640, 0, 2), (640, 0, -1)]:
        assert lib.lp_view_grid(tile, ov, full, 2048, 2048, C.byref(n), None, 0) == _ffi.LP_ERR_ARG, (tile, ov, full)
    for H, W in [(0, 100), (100, 0), (-5, 100)]:
        assert lib.lp_view_grid(640, 0, 1, H, W, C.byref(n), None, 0) == _ffi.LP_ERR_ARG
    assert lib.lp_view_grid(640, 0, 1, 2048, 2048, None, None, 0) == _ffi.LP_ERR_ARG
    buf = (C.c_int * 4)()
    assert lib.lp_view_grid(640, 128, 1, 2048, 2048, C.byref(n), buf, 1) == _ffi.LP_ERR_ARG   # no room
    r = C.c_float()
    geo = lambda H, W, v: lib.lp_view_geometry(640, H, W, (C.c_int * 4)(*v), C.byref(r), None, None, None, None, None, None)
    assert geo(480, 640, (0, 0, 640, 480)) == _ffi.LP_OK and geo(480, 640, (-1, -1, 0, 0)) == _ffi.LP_OK
    for v in [(1, 0, 640, 480), (0, 1, 640, 480), (0, 0, 15, 100), (0, 0, 100, 15), (-2, 0, 100, 100), (0, -1, 100, 100),
              (600, 0, 41, 100), (0, 470, 100, 11)]:
        assert geo(480, 640, v) == _ffi.LP_ERR_ARG, v
        assert lib.lp_last_error()
    assert lib.lp_view_geometry(640, 480, 640, None, C.byref(r), None, None, None, None, None, None) == _ffi.LP_ERR_ARG
    assert lib.lp_view_geometry(0, 480, 640, (C.c_int * 4)(0, 0, 64, 64), C.byref(r), None, None, None, None, None, None) == _ffi.LP_ERR_ARG
    for v in [(1, 0, 640, 480), (0, 0, 15, 100), (-2, 0, 100, 100)]:
        with pytest.raises(ValueError):
            V.view_geometry(640, 480, 640, v)


def test_merge_sign_seen_at_half_scale_and_native_collapses():
    """one sign of a 2048 x 2048 frame seen by a half-scale 1280 window (view 0) and by a native 640 window (view 1): each
    view's decoded box goes through its own un-letterbox in fp32, lands within a pixel of the other, and the frame NMS keeps
    one -- the higher score, whichever view it comes from; a second sign only the native view sees stays"""
    S, H, W = 640, 2048, 2048
    views = [(768, 768, 1280, 1280), (1024, 1024, 640, 640)]
    geo = [V.view_geometry(S, H, W, v) for v in views]
    assert float(geo[0]["ratio"]) == 0.5 and float(geo[1]["ratio"]) == 1.0
    sign = np.array([1100.0, 1200.0, 1160.0, 1260.0])
    far = np.array([1500.0, 1500.0, 1530.0, 1530.0])

    def out0_for(g, boxes, scores):   # the [4 + nc, A] head output that decodes to these frame boxes in view g
        o = np.zeros((5, 8), np.float32)
        for a, (b, s) in enumerate(zip(boxes, scores)):
            v = b * float(g["ratio"]) + np.array([g["pad_w"], g["pad_h"]] * 2, np.float64)
            o[:4, a] = [(v[0] + v[2]) / 2, (v[1] + v[3]) / 2, v[2] - v[0], v[3] - v[1]]
            o[4, a] = s
        return o

    cands = [T.view_candidates(out0_for(geo[0], [sign + 0.4], [0.8]), (H, W), geo[0]["ratio"], (geo[0]["pad_w"], geo[0]["pad_h"]), 0.25),
             T.view_candidates(out0_for(geo[1], [sign, far], [0.6, 0.5]), (H, W), geo[1]["ratio"], (geo[1]["pad_w"], geo[1]["pad_h"]), 0.25)]
    b = np.concatenate([c[0] for c in cands]); s = np.concatenate([c[1] for c in cands]); c = np.concatenate([c[2] for c in cands])
    v = np.array([0, 1, 1]); a = np.concatenate([c[3] for c in cands])
    assert np.abs(b[0] - (sign + 0.4)).max() < 1e-3 and np.abs(b[1] - sign).max() < 1e-3   # both in frame pixels
    k = T.merge(b, s, c, v, a, 0.45)
    assert k.tolist() == [0, 2]       # the half-scale sighting wins the sign, the far sign stays
    s2 = s.copy(); s2[1] = 0.9
    assert T.merge(b, s2, c, v, a, 0.45).tolist() == [1, 2]   # ... or the native one, when it scores higher


def test_cli_view_flags():
    from litepi import e2e
    assert e2e.parse_views("full; 0,540,1920,540 ;768,768,1280,1280") == ["full", (0, 540, 1920, 540), (768, 768, 1280, 1280)]
    for bad in ("", "full;1,2,3", "a,b,c,d", "full;;"):
        with pytest.raises(SystemExit):
            e2e.parse_views(bad)
    p = e2e.build_parser()
    a = p.parse_args(["--view_tile", "1280", "--view_overlap", "256"])
    assert (a.view_tile, a.view_overlap, a.view_full_frame, a.views, a.tile_overlap) == (1280, 256, 1, None, None)
    for argv in (["--view_tile", "1280", "--tile_overlap", "128"], ["--views", "full", "--view_tile", "640"], ["--views", "full", "--tile_overlap", "0"],
                 ["--views", "full;1,2"]):
        with pytest.raises(SystemExit):
            e2e.check_frame_args(p.parse_args(argv))
