"""Tiled inference on the CPU: the view grid rule, the library's lp_tile_grid (host only) against it, and the merge oracle."""
import ctypes as C

import numpy as np
import pytest

import tiling_ref as T
from oracle import postprocess_ref as P


@pytest.mark.parametrize("H,W,overlap,xs,ys", [
    (2048, 2048, 0, [0, 640, 1280, 1408], [0, 640, 1280, 1408]),
    (2048, 2048, 128, [0, 512, 1024, 1408], [0, 512, 1024, 1408]),
    (2048, 2048, 170, [0, 470, 940, 1408], [0, 470, 940, 1408]),
    (2048, 2048, 171, [0, 469, 938, 1407, 1408], [0, 469, 938, 1407, 1408]),
    (681, 1198, 128, [0, 512, 558], [0, 41]),
    (2000, 500, 128, [0], [0, 512, 1024, 1360]),
    (640, 640, 128, [0], [0]),
    (641, 641, 128, [0, 1], [0, 1]),
])
def test_grid_rule_worked_cases(H, W, overlap, xs, ys):
    from litepi.backend import tile_grid   # the library's lp_tile_grid (host only)
    assert T.tile_axis(W, 640, overlap) == xs and T.tile_axis(H, 640, overlap) == ys
    views = T.tile_grid(640, H, W, overlap, True)
    assert tile_grid(640, H, W, overlap, True) == views and tile_grid(640, H, W, overlap, False) == T.tile_grid(640, H, W, overlap, False)
    if len(xs) * len(ys) == 1:
        assert views == [(-1, -1, W, H)]
    else:
        assert views[0] == (-1, -1, W, H)
        assert views[1:] == [(x, y, 640, 640) for y in ys for x in xs]
        assert T.tile_grid(640, H, W, overlap, False) == views[1:]


def test_grid_2048_overlap128_is_17_views():
    from litepi.backend import tile_grid
    assert len(T.tile_grid(640, 2048, 2048, 128, True)) == len(tile_grid(640, 2048, 2048, 128, True)) == 17


@pytest.mark.parametrize("S", [640, 320])
@pytest.mark.parametrize("full", [True, False])
def test_lp_tile_grid_matches_python(S, full):
    from litepi import _ffi
    from litepi.backend import tile_grid
    for H, W in [(2048, 2048), (681, 1198), (2000, 500), (S, S), (S + 1, S + 1), (1, 5000), (1024, 1280)]:
        for ov in (0, 128, 170, 171, S - 1):
            assert tile_grid(S, H, W, ov, full) == T.tile_grid(S, H, W, ov, full), (H, W, ov)
    lib = _ffi.load_library()
    t = _ffi.LpTiling()
    n = C.c_int()
    for bad in (-1, S):
        t.overlap, t.full_frame = bad, 1
        assert lib.lp_tile_grid(S, C.byref(t), 100, 100, C.byref(n), None, 0) == _ffi.LP_ERR_ARG
    t.overlap, t.full_frame = 128, 2
    assert lib.lp_tile_grid(S, C.byref(t), 100, 100, C.byref(n), None, 0) == _ffi.LP_ERR_ARG
    t.full_frame = 1
    buf = (C.c_int * 4)()
    assert lib.lp_tile_grid(S, C.byref(t), 2048, 2048, C.byref(n), buf, 1) == _ffi.LP_ERR_ARG   # no room


def _box(x, y, s=30.0):
    return [x, y, x + s, y + s]


def test_merge_duplicate_in_overlap_collapses():
    # the same sign seen by view 1 and view 2 (neighbouring crops), one other box
    b = np.array([_box(600, 100), _box(100, 100), _box(601, 100)], np.float32)
    k = T.merge(b, [0.9, 0.5, 0.8], [0, 0, 0], [1, 1, 2], [10, 20, 5], 0.45)
    assert k.tolist() == [0, 1]


def test_merge_exact_ties_keep_higher_view():
    b = np.array([_box(600, 100), _box(600.5, 100)], np.float32)
    k = T.merge(b, [0.7, 0.7], [0, 0], [1, 2], [50, 3], 0.45)
    assert k.tolist() == [1]   # view 2 wins the tie although its anchor is lower
    k = T.merge(b, [0.7, 0.7], [0, 0], [2, 2], [3, 50], 0.45)
    assert k.tolist() == [1]   # same view: the higher anchor


def test_merge_max_det_over_union():
    rng = np.random.default_rng(0)
    n = 40
    xy = rng.uniform(0, 2000, (n, 2))
    b = np.concatenate([xy, xy + 20], 1).astype(np.float32)
    s = rng.uniform(0.3, 1, n).astype(np.float32)
    c = rng.integers(0, 3, n)
    v = np.sort(rng.integers(0, 4, n))
    a = np.arange(n)
    full = T.merge(b, s, c, v, a, 0.45)
    cut = T.merge(b, s, c, v, a, 0.45, max_det=7)
    assert len(cut) == 7 and set(cut) <= set(full)
    assert sorted(s[cut].tolist(), reverse=True) == sorted(s[full].tolist(), reverse=True)[:7]
    assert [x for x in full if x in set(cut)] == cut.tolist()   # output order kept


def test_merge_one_view_equals_postprocess():
    rng = np.random.default_rng(3)
    A, nc = 500, 3
    out0 = np.zeros((4 + nc, A), np.float32)
    out0[0] = rng.uniform(0, 640, A); out0[1] = rng.uniform(0, 640, A)
    out0[2] = rng.uniform(5, 80, A); out0[3] = rng.uniform(5, 80, A)
    out0[4:] = rng.uniform(0, 1, (nc, A))
    out0[4:, ::7] = 0.75   # exact ties
    r, pad = 0.3125, (0.0, 0.0 + 140.0)
    eb, es, ec = P.postprocess(out0, (1400, 2048), r, pad, 0.25, 0.45)
    b, s, c, a = T.view_candidates(out0, (1400, 2048), r, pad, 0.25)
    k = T.merge(b, s, c, np.zeros(len(a), np.int64), a, 0.45)
    assert np.array_equal(b[k], eb.astype(np.float32)) and np.array_equal(s[k], es) and np.array_equal(c[k], ec)
