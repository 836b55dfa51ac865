"""CPU tests of the focus rule (tests/focus_ref.py) against hand-worked cases, and of the library's host-only entry points:
the header's declarations, the exported symbols, the struct size and lp_focus_config_check."""
import ctypes as C
import os

import numpy as np
import pytest

import focus_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, S = 704, 896, 320
CFG = dict(side_min=320, sweep_overlap=64)
NEW = ("lp_focus_default_config", "lp_focus_config_check", "lp_focus_create", "lp_focus_destroy", "lp_focus_plan", "lp_focus_state",
       "lp_run_focus_device", "lp_run_focus")


def track(slot, box, vel=(0, 0, 0, 0), hits=3, missed=0):
    return (slot, *box, *vel, hits, missed)


def plan1(ref, rows, h=H, w=W, **kw):
    return [tuple(v) for v in ref.plan({0: R.make_tracks(rows)}, [h], [w], **kw)[0].tolist()]


# ---------------------------------------------------------------------------- the library's host side
def test_header_declares_and_library_exports_the_focus_calls():
    from litepi import _ffi

    text = open(os.path.join(ROOT, "include", "litepi.h")).read()
    lib = _ffi.load_library()
    for s in NEW:
        assert s + "(" in text, f"{s} is not declared in include/litepi.h"
        assert s in _ffi.SYMBOLS
        getattr(lib, s)
    assert "typedef struct lp_focus_config" in text
    assert lib.lp_version() == 310


def test_config_struct_defaults_and_check():
    from litepi import _ffi
    from litepi.backend import focus_config, focus_config_check

    assert C.sizeof(_ffi.LpFocusConfig) == 64
    c = focus_config()
    assert (c.slots, c.side_min, c.side_max, c.border, c.sweep, c.sweep_overlap) == (3, 0, 0, 16, 1, 0)
    assert (c.margin, c.small_px) == (2.0, 32.0) and list(c.reserved) == [0] * 8
    assert {k: (int(getattr(c, k)) if k not in ("margin", "small_px") else getattr(c, k)) for k in R.DEFAULTS} == R.DEFAULTS
    assert focus_config_check(c, 640) == 0 and focus_config_check(c, 64) == 0
    assert focus_config_check(None, 640) == _ffi.LP_ERR_ARG
    bad = [dict(slots=0), dict(slots=17), dict(side_min=15), dict(side_min=-1), dict(side_max=-1), dict(side_min=700, side_max=699),
           dict(side_min=1300), dict(side_max=8 * 640 + 1), dict(margin=0.99), dict(margin=float("nan")), dict(small_px=0.0),
           dict(small_px=-1.0), dict(small_px=float("nan")), dict(border=-1), dict(sweep=2), dict(sweep=-1), dict(sweep_overlap=-1),
           dict(sweep_overlap=640), dict(side_min=32, sweep_overlap=32)]
    for kw in bad:
        assert focus_config_check(focus_config(**kw), 640) == _ffi.LP_ERR_ARG, kw
    good = [dict(slots=1), dict(slots=16), dict(side_min=16, side_max=16), dict(side_max=8 * 640), dict(margin=1.0), dict(border=0),
            dict(sweep=0), dict(sweep_overlap=639), dict(side_min=1280)]
    for kw in good:
        assert focus_config_check(focus_config(**kw), 640) == 0, kw
    for i in range(8):
        c = focus_config()
        c.reserved[i] = 1
        assert focus_config_check(c, 640) == _ffi.LP_ERR_ARG
    with pytest.raises(TypeError):
        focus_config(slot=3)


# ---------------------------------------------------------------------------- the rule, by hand
def test_sweep_grid_and_cursor():
    G = R.view_grid(320, 64, H, W)
    assert len(G) == 12
    assert sorted({g[0] for g in G}) == [0, 256, 512, 576] and sorted({g[1] for g in G}) == [0, 256, 384]
    assert G[:5] == [(0, 0, 320, 320), (256, 0, 320, 320), (512, 0, 320, 320), (576, 0, 320, 320), (0, 256, 320, 320)]
    ref = R.FocusRef(S, slots=5, **CFG)
    seen, cursors = [], []
    for _ in range(3):
        seen += plan1(ref, [])
        cursors.append(ref.state[0]["cursor"])
    assert cursors == [5, 10, 3]
    assert set(seen) == set(G) and seen[:12] == G and seen[12:] == G[:3]
    assert ref.state[0]["unserved"] == 0


def test_cover_border_and_one_pixel_outside():
    ref = R.FocusRef(S, slots=3, sweep=0, **CFG)
    first = track(0, (400, 300, 440, 340), hits=9)
    # side = ceil(2 * 40) = 80 -> side_min; centre (420, 320)
    assert plan1(ref, [first]) == [(260, 160, 320, 320), (0, 0, 0, 0), (0, 0, 0, 0)]
    # the covered region of that window is [276, 564] x [176, 464]
    inside = track(1, (276, 176, 300, 200))
    assert plan1(ref, [first, inside]) == [(260, 160, 320, 320), (0, 0, 0, 0), (0, 0, 0, 0)]
    outside = track(1, (275, 176, 300, 200))   # centre (287, 188)
    assert plan1(ref, [first, outside]) == [(260, 160, 320, 320), (127, 28, 320, 320), (0, 0, 0, 0)]
    far_edge = track(1, (540, 440, 564, 464))
    assert plan1(ref, [first, far_edge])[1] == (0, 0, 0, 0)
    assert plan1(ref, [first, track(1, (540, 440, 565, 464))])[1] != (0, 0, 0, 0)
    assert ref.state[0]["unserved"] == 0


def test_frame_corner_is_clamped_and_covered_at_the_edge():
    ref = R.FocusRef(S, slots=2, sweep=0, **CFG)
    corner = track(0, (0, 0, 30, 30), hits=5)
    assert plan1(ref, [corner]) == [(0, 0, 320, 320), (0, 0, 0, 0)]
    # a box that touches the frame's edge is inside no border there, and still covered
    assert plan1(ref, [corner, track(1, (2, 0, 20, 20))]) == [(0, 0, 320, 320), (0, 0, 0, 0)]
    low = track(0, (870, 680, 896, 704), hits=5)
    assert plan1(ref, [low]) == [(576, 384, 320, 320), (0, 0, 0, 0)]
    assert plan1(ref, [low, track(1, (880, 690, 896, 704))]) == [(576, 384, 320, 320), (0, 0, 0, 0)]
    # a prediction that leaves the frame is clipped to it first
    out = track(0, (-20, -20, 30, 30), hits=5)
    assert plan1(ref, [out]) == [(0, 0, 320, 320), (0, 0, 0, 0)]
    assert plan1(ref, [track(0, (-50, -50, -10, -10))]) == [(0, 0, 0, 0)] * 2


def test_unserved_and_hits_order():
    ref = R.FocusRef(S, slots=1, sweep=0, **CFG)
    a, b = track(0, (100, 100, 130, 130), hits=2), track(1, (700, 500, 730, 530), hits=7)
    assert plan1(ref, [a, b]) == [(555, 355, 320, 320)]
    assert ref.state[0] == {"cursor": 0, "unserved": 1}
    # ties go to the lower slot
    a = track(0, (100, 100, 130, 130), hits=7)
    assert plan1(ref, [a, b]) == [(0, 0, 320, 320)]
    assert ref.state[0]["unserved"] == 2
    assert plan1(ref, [a, b], advance=False) == [(0, 0, 320, 320)] and ref.state[0]["unserved"] == 2


def test_nan_never_asks_and_large_boxes_do_not_ask():
    ref = R.FocusRef(S, slots=2, sweep=0, **CFG)
    nan = float("nan")
    for box in [(nan, 100, 130, 130), (100, nan, 130, 130), (100, 100, nan, 130), (100, 100, 130, nan)]:
        assert plan1(ref, [track(0, box)]) == [(0, 0, 0, 0)] * 2
    assert plan1(ref, [track(0, (100, 100, 130, 130), vel=(nan, 0, 0, 0))]) == [(0, 0, 0, 0)] * 2
    # rf = 320 / 896: the longer side asks below 89.6 pixels
    assert plan1(ref, [track(0, (100, 100, 189, 130))])[0] != (0, 0, 0, 0)
    assert plan1(ref, [track(0, (100, 100, 190, 130))]) == [(0, 0, 0, 0)] * 2
    assert plan1(ref, [track(0, (100, 100, 100, 130))]) == [(0, 0, 0, 0)] * 2   # no width


def test_small_frame_has_no_sweep():
    ref = R.FocusRef(S, slots=4, **CFG)
    assert R.view_grid(320, 64, 300, 320) == []
    assert plan1(ref, [], h=300, w=320) == [(0, 0, 0, 0)] * 4
    assert ref.state[0] == {"cursor": 0, "unserved": 0}
    # one pixel more and two windows sweep it
    assert plan1(ref, [], h=300, w=321) == [(0, 0, 320, 300), (1, 0, 320, 300), (0, 0, 0, 0), (0, 0, 0, 0)]
    assert ref.state[0]["cursor"] == 0


def test_j_predicts_one_frame_further():
    ref = R.FocusRef(S, n_streams=2, slots=1, sweep=0, **CFG)
    t = R.make_tracks([track(0, (300, 300, 330, 330), vel=(10, 0, 10, 0), missed=1)])
    got = ref.plan({0: t, 1: t}, [H, H, H], [W, W, W], stream_ids=[0, 1, 0])
    # dt = missed + 1 + j: centre x 315 + 20 (j = 0) and 315 + 30 (j = 1)
    assert got[:, 0].tolist() == [[175, 155, 320, 320], [175, 155, 320, 320], [185, 155, 320, 320]]
    still = R.FocusRef(S, motion=0, slots=1, sweep=0, **CFG)
    assert still.plan({0: t}, [H, H], [W, W])[:, 0].tolist() == [[155, 155, 320, 320]] * 2


def test_side_follows_margin_and_both_clamps():
    def side(m, **kw):
        ref = R.FocusRef(S, slots=1, sweep=0, small_px=1000.0, **dict(CFG, **kw))
        return plan1(ref, [track(0, (200, 200, 200 + m, 210))])[0][2:]

    assert side(40) == (320, 320)          # 80 -> side_min
    assert side(200) == (400, 400)         # margin 2
    assert side(150, margin=3.0) == (450, 450)
    assert side(100.2, margin=2.5) == (320, 320) and side(130.1, margin=2.5) == (326, 326)   # ceil
    assert side(400) == (640, 640)         # 800 -> side_max = 2 * det_input
    assert side(400, side_max=700) == (700, 700)
    assert side(400, side_max=2000) == (800, 704)   # the frame's height bounds the window


def test_sweep_follows_the_placed_windows():
    ref = R.FocusRef(S, slots=3, **CFG)
    G = R.view_grid(320, 64, H, W)
    assert plan1(ref, [track(0, (400, 300, 440, 340))]) == [(260, 160, 320, 320), G[0], G[1]]
    assert plan1(ref, []) == [G[2], G[3], G[4]]
    assert ref.state[0]["cursor"] == 5
