"""CPU tests of the frame NMS of views with a match metric and a box-union merge (include/litepi.h "frame NMS of views"):
the C ABI's host side (symbols, struct size, lp_view_merge_check), the NumPy statement of the rule (tests/view_merge_ref.py)
against tests/tiling_ref.py and on hand-built cases, and the refusals of the pipeline and command-line options."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import tiling_ref as T
import view_merge_ref as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lp_view_merge_default", "lp_view_merge_check", "lp_set_view_merge")


def _lib():
    from litepi import _ffi
    return _ffi.load_library()


# ---------------------------------------------------------------------------- 1. the C ABI's host side
def test_header_declares_and_library_exports_the_symbols():
    from litepi import _ffi
    header = open(os.path.join(ROOT, "include", "litepi.h")).read()
    declared = set(re.findall(r"\b(lp_[a-z0-9_]+)\s*\(", header))
    lib = _lib()
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in litepi.h"
        assert name in _ffi.SYMBOLS
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"enum lp_match \{ LP_MATCH_IOU = 0, LP_MATCH_IOS = 1 \};", header)
    assert re.search(r"enum lp_merge \{ LP_MERGE_SUPPRESS = 0, LP_MERGE_UNION = 1 \};", header)
    assert re.search(r"#define LP_ABI_VERSION 310\b", header) and lib.lp_version() == 310
    assert (_ffi.LP_MATCH_IOU, _ffi.LP_MATCH_IOS, _ffi.LP_MERGE_SUPPRESS, _ffi.LP_MERGE_UNION) == (0, 1, 0, 1)


def test_sizeof_lp_view_merge_is_32():
    from litepi import _ffi
    assert ctypes.sizeof(_ffi.LpViewMerge) == 32
    header = open(os.path.join(ROOT, "include", "litepi.h")).read()
    body = re.search(r"typedef struct lp_view_merge \{(.*?)\} lp_view_merge;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int|float)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    assert [(t, n, int(k or 1)) for t, n, k in fields] == [("int", "metric", 1), ("int", "mode", 1), ("float", "threshold", 1),
                                                          ("int", "reserved", 5)]
    assert [(n, ctypes.sizeof(t)) for n, t in _ffi.LpViewMerge._fields_] == [("metric", 4), ("mode", 4), ("threshold", 4), ("reserved", 20)]


def test_view_merge_default_and_check():
    from litepi import _ffi
    lib = _lib()
    m = _ffi.LpViewMerge(7, 7, 0.5, (ctypes.c_int * 5)(1, 2, 3, 4, 5))
    lib.lp_view_merge_default(ctypes.byref(m))
    assert (m.metric, m.mode, m.threshold, list(m.reserved)) == (_ffi.LP_MATCH_IOU, _ffi.LP_MERGE_SUPPRESS, 0.0, [0] * 5)
    assert lib.lp_view_merge_check(ctypes.byref(m)) == _ffi.LP_OK

    def status(**kw):
        c = _ffi.LpViewMerge()
        lib.lp_view_merge_default(ctypes.byref(c))
        for k, v in kw.items():
            if k.startswith("reserved"):
                c.reserved[int(k[8:])] = v
            else:
                setattr(c, k, v)
        return lib.lp_view_merge_check(ctypes.byref(c))

    for metric, mode in itertools.product((0, 1), (0, 1)):
        for thr in (0.0, 1e-6, 0.45, 0.999999):
            assert status(metric=metric, mode=mode, threshold=thr) == _ffi.LP_OK, (metric, mode, thr)
    for bad in (dict(metric=2), dict(metric=-1), dict(mode=2), dict(mode=-1), dict(threshold=float("nan")), dict(threshold=-0.25),
                dict(threshold=-1e-30), dict(threshold=1.0), dict(threshold=7.0), dict(threshold=float("inf")),
                *[{f"reserved{k}": 1} for k in range(5)]):
        assert status(**bad) == _ffi.LP_ERR_ARG, bad
    assert lib.lp_view_merge_check(None) == _ffi.LP_ERR_ARG
    assert "null" in lib.lp_last_error().decode()
    # the setter checks before it looks at the handle
    assert lib.lp_set_view_merge(None, None) == _ffi.LP_ERR_ARG


def test_backend_names():
    from litepi import _ffi
    from litepi.backend import view_merge_check, view_merge_config
    m = view_merge_config("ios", "union", 0.6)
    assert (m.metric, m.mode, m.threshold) == (_ffi.LP_MATCH_IOS, _ffi.LP_MERGE_UNION, np.float32(0.6)) and view_merge_check(m) == 0
    m = view_merge_config()
    assert (m.metric, m.mode, m.threshold) == (0, 0, 0.0)
    for bad in (dict(match="giou"), dict(merge="wbf")):
        with pytest.raises(ValueError):
            view_merge_config(**bad)
    assert view_merge_check(view_merge_config(threshold=1.5)) == _ffi.LP_ERR_ARG


# ---------------------------------------------------------------------------- 2. the ref against tiling_ref
def _random_views(rng, n_views, per_view, nc, H=2048, W=2048, ties=True):
    """tests/test_gpu_tiling.py::_random_views, copied"""
    bs, ss, cs, vs, an = [], [], [], [], []
    centres = rng.uniform(0, min(H, W), (max(4, per_view // 4), 2))
    for v in range(n_views):
        a = np.sort(rng.choice(8400, size=per_view, replace=False))
        c = centres[rng.integers(0, len(centres), per_view)] + rng.normal(0, 6, (per_view, 2))
        wh = rng.uniform(15, 60, (per_view, 2))
        b = np.concatenate([c - wh / 2, c + wh / 2], 1).clip(0, [W, H, W, H]).astype(np.float32)
        s = rng.uniform(0.25, 1.0, per_view).astype(np.float32)
        if ties:
            s[::5] = np.float32(0.625)   # exact ties inside and across views
        bs.append(b); ss.append(s); cs.append(rng.integers(0, nc, per_view)); vs.append(np.full(per_view, v)); an.append(a)
    return (np.concatenate(bs), np.concatenate(ss), np.concatenate(cs).astype(np.int32), np.concatenate(vs).astype(np.int32),
            np.concatenate(an).astype(np.int32))


@pytest.mark.parametrize("n_views,per_view", [(3, 10), (2, 32), (2, 300), (5, 200), (17, 120)])
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("max_det", [None, 23])
def test_ref_iou_suppress_is_tiling_ref(n_views, per_view, nc, max_det):
    rng = np.random.default_rng(n_views * 10 + nc)
    b, s, c, v, a = _random_views(rng, n_views, per_view, nc)
    exp = T.merge(b, s, c, v, a, 0.45, max_det)
    k, out = VM.merge(b, s, c, v, a, 0.45, max_det)
    assert np.array_equal(k, exp)
    assert np.array_equal(out.view(np.uint32), b[k].view(np.uint32))
    # suppress emits the keepers' own boxes under either metric; union keeps the keepers of suppress
    for metric in (VM.IOU, VM.IOS):
        ks, outs = VM.merge(b, s, c, v, a, 0.45, max_det, metric, VM.SUPPRESS)
        ku, outu = VM.merge(b, s, c, v, a, 0.45, max_det, metric, VM.UNION)
        assert np.array_equal(ks, ku) and np.array_equal(outs, b[ks])
        assert (outu[:, :2] <= b[ku][:, :2]).all() and (outu[:, 2:] >= b[ku][:, 2:]).all()
        assert (outu != b[ku]).any(), "no box grew: the union case is vacuous"


# ---------------------------------------------------------------------------- 3. hand-built cases
WHOLE = [100.0, 100.0, 180.0, 160.0]
# the same sign cut by the borders of two views that overlap by 20 pixels (one ends at x = 130, the next begins at x = 110):
# IoU with the whole box 0.375 and 0.875, with each other 0.25; IoS with the whole box 1, with each other 20 / 30
LEFT = [100.0, 100.0, 130.0, 160.0]
RIGHT = [110.0, 100.0, 180.0, 160.0]


def _views_of(boxes, scores, classes=None, views=None, anchors=None):
    n = len(boxes)
    return (np.array(boxes, np.float32), np.array(scores, np.float32), np.zeros(n, np.int32) if classes is None else np.array(classes, np.int32),
            np.arange(n, dtype=np.int32) if views is None else np.array(views, np.int32),
            np.full(n, 5, np.int32) if anchors is None else np.array(anchors, np.int32))


@pytest.mark.parametrize("scores", list(itertools.permutations((0.9, 0.8, 0.7))))
def test_whole_box_and_two_cut_halves(scores):
    args = _views_of([WHOLE, LEFT, RIGHT], scores)
    k, out = VM.merge(*args, 0.45, None, VM.IOS, VM.UNION)
    assert len(k) == 1 and k[0] == int(np.argmax(scores)), "IoS + union: one box whichever part scored highest"
    assert np.array_equal(out[0], np.array(WHOLE, np.float32))
    k, out = VM.merge(*args, 0.45, None, VM.IOU, VM.SUPPRESS)
    assert len(k) in (2, 3), "IoU + suppress: the duplicate the feature removes"
    assert np.array_equal(k, T.merge(*args, 0.45)) and np.array_equal(out, args[0][k])
    # IoS alone drops the duplicates but may keep a cut box
    k, out = VM.merge(*args, 0.45, None, VM.IOS, VM.SUPPRESS)
    assert len(k) == 1 and np.array_equal(out[0], args[0][int(np.argmax(scores))])


def test_disjoint_parts_under_a_part_that_scores_highest():
    """The walk is not iterated and matches the keeper's own box: with views that do not overlap, the two parts of a sign share
    no pixel, so a part that outscores the whole box takes the whole box and leaves the other part a keeper of its own."""
    l, r = [100.0, 100.0, 128.0, 160.0], [128.0, 100.0, 180.0, 160.0]
    k, out = VM.merge(*_views_of([WHOLE, l, r], [0.8, 0.9, 0.7]), 0.45, None, VM.IOS, VM.UNION)
    assert k.tolist() == [1, 2] and out.tolist() == [WHOLE, r]
    k, out = VM.merge(*_views_of([WHOLE, l, r], [0.9, 0.8, 0.7]), 0.45, None, VM.IOS, VM.UNION)
    assert k.tolist() == [0] and out.tolist() == [WHOLE]


def test_chain_is_not_transitive():
    a, b, c = [0, 0, 100, 100], [50, 0, 150, 100], [100, 0, 200, 100]   # a ~ b (1/3), b ~ c, a and c only touch
    args = _views_of([a, b, c], [0.9, 0.8, 0.7])
    for metric in (VM.IOU, VM.IOS):
        k, out = VM.merge(*args, 0.3, None, metric, VM.UNION)
        assert k.tolist() == [0, 2]
        assert out.tolist() == [[0, 0, 150, 100], [100, 0, 200, 100]], "c stays a keeper although it overlaps a's union"
    # with b first in O it takes both
    k, out = VM.merge(*_views_of([a, b, c], [0.8, 0.9, 0.7]), 0.3, None, VM.IOU, VM.UNION)
    assert k.tolist() == [1] and out.tolist() == [[0, 0, 200, 100]]


def test_exact_score_ties_follow_view_then_anchor():
    box = [600, 100, 640, 140]
    grown = [590, 100, 640, 140]
    b, s, c, v, a = _views_of([grown, box, box, box], [0.5] * 4, views=[0, 1, 2, 2], anchors=[8999, 17, 3, 4])
    for metric, mode in itertools.product((VM.IOU, VM.IOS), (VM.SUPPRESS, VM.UNION)):
        k, out = VM.merge(b, s, c, v, a, 0.45, None, metric, mode)
        assert k.tolist() == [3], "the highest (view, anchor) is the keeper"
        assert out[0].tolist() == (grown if mode == VM.UNION else box)
    assert VM.order(s, c, v, a).tolist() == [3, 2, 1, 0]


def test_equal_boxes_of_different_classes_never_match():
    args = _views_of([WHOLE] * 3, [0.9, 0.8, 0.7], classes=[2, 0, 1])
    for metric, mode in itertools.product((VM.IOU, VM.IOS), (VM.SUPPRESS, VM.UNION)):
        k, out = VM.merge(*args, 0.45, None, metric, mode)
        assert k.tolist() == [1, 2, 0] and np.array_equal(out, args[0][k])   # class ascending


def test_zero_area_box_never_matches_under_ios():
    line = [120.0, 100.0, 120.0, 160.0]    # inside WHOLE, no area: inter = 0, m = 0 / 1e-6 = 0
    point = [150.0, 130.0, 150.0, 130.0]
    for scores in itertools.permutations((0.9, 0.8, 0.7)):
        args = _views_of([WHOLE, line, point], scores)
        k, out = VM.merge(*args, 0.45, None, VM.IOS, VM.UNION, threshold=1e-6)
        assert sorted(k.tolist()) == [0, 1, 2] and np.array_equal(out, args[0][k])
    assert VM.match_value(np.array(WHOLE, np.float32), np.array([line, point, line], np.float32), VM.IOS).tolist() == [0, 0, 0]
    assert VM.match_value(np.array(line, np.float32), np.array([line], np.float32), VM.IOS).tolist() == [0]


def test_configured_threshold_replaces_the_calls_iou():
    args = _views_of([[0, 0, 100, 100], [50, 0, 150, 100]], [0.9, 0.8])   # IoU 1/3, IoS 1/2
    assert len(VM.merge(*args, 0.45, None, VM.IOU, VM.UNION)[0]) == 2
    assert len(VM.merge(*args, 0.45, None, VM.IOU, VM.UNION, threshold=0.3)[0]) == 1
    assert len(VM.merge(*args, 0.3, None, VM.IOU, VM.UNION, threshold=0.45)[0]) == 2
    assert len(VM.merge(*args, 0.3, None, VM.IOU, VM.UNION, threshold=0.0)[0]) == 1


# ---------------------------------------------------------------------------- 4. refusals without a view family
@pytest.mark.parametrize("opt", [dict(view_match="ios"), dict(view_merge="union"), dict(view_match_thr=0.5),
                                 dict(view_match="ios", view_merge="union", view_match_thr=0.3), dict(view_match="iou"), dict(view_merge="nms")])
def test_pipeline_view_merge_options_need_a_view_family(opt):
    """ValueError before anything is loaded or any handle is created (the model files do not exist)"""
    from litepi import HybridPipeline
    with pytest.raises(ValueError, match="need one of tile_overlap, views, view_tile or focus"):
        HybridPipeline("none.param", "none.bin", "none.pth", "shufflenetv2", **opt)


def test_pipeline_view_merge_options_are_checked_before_a_handle():
    from litepi import HybridPipeline
    for opt in (dict(view_match="giou"), dict(view_merge="wbf"), dict(view_match_thr=1.0), dict(view_match_thr=-0.1),
                dict(view_match_thr=float("nan"))):
        with pytest.raises(ValueError):
            HybridPipeline("none.param", "none.bin", "none.pth", "shufflenetv2", tile_overlap=128, **opt)


def test_cli_view_merge_options():
    from litepi import e2e
    p = e2e.build_parser()
    a = p.parse_args([])
    assert (a.view_match, a.view_merge, a.view_match_thr) == (None, None, None)
    e2e.check_frame_args(a)
    for extra in (["--view_match", "ios"], ["--view_merge", "union"], ["--view_match_thr", "0.5"],
                  ["--view_match", "ios", "--view_merge", "union", "--view_match_thr", "0.3"]):
        with pytest.raises(SystemExit, match="need one of --tile_overlap"):
            e2e.check_frame_args(p.parse_args(extra))
        for family in (["--tile_overlap", "64"], ["--view_tile", "960"], ["--views", "full"]):
            e2e.check_frame_args(p.parse_args(extra + family))
    for bad in (["--view_match", "giou"], ["--view_merge", "wbf"], ["--view_match_thr", "high"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for thr in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit, match="outside"):
            e2e.check_frame_args(p.parse_args(["--tile_overlap", "64", "--view_match_thr", thr]))
