"""Groundwork of a rectangular detector input, on the CPU: the pure-host geometry (lp_letterbox_geometry)
against the Python restatement of the reference's letterbox(img, (SH, SW)) in tests/rect_ref.py, and the exporter's anchor
tables, Reshape extents and oracle forward at a (rows, columns) size.  Shapes are (rows, columns)."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import rect_ref as R

DET_SIZES = [(640, 640), (384, 640), (640, 384), (320, 640), (224, 416)]
FRAMES = [(1080, 1920), (720, 1280), (480, 640), (640, 360), (100, 37), None, (2048, 2048)]   # None: the detector input's own size
INT_KEYS = ("new_w", "new_h", "top", "left")
FLOAT_KEYS = ("ratio", "pad_w", "pad_h")


@pytest.mark.parametrize("det", DET_SIZES, ids=[f"{h}x{w}" for h, w in DET_SIZES])
def test_letterbox_geometry_equals_the_reference_rule(det):
    from litepi.backend import letterbox_geometry, view_geometry
    SH, SW = det
    for hw in FRAMES:
        H, W = hw or det
        got, want = letterbox_geometry(SH, SW, H, W), R.letterbox_geometry(SH, SW, H, W)
        for k in INT_KEYS:
            assert got[k] == want[k], (det, H, W, k, got[k], want[k])
        for k in FLOAT_KEYS:
            assert np.float32(got[k]).view(np.uint32) == np.float32(want[k]).view(np.uint32), (det, H, W, k, got[k], want[k])
        if hw is None:   # an image of the input's size is the identity
            assert (got["new_w"], got["new_h"], got["top"], got["left"]) == (SW, SH, 0, 0) and got["ratio"] == 1.0
        if SH == SW:     # the square case is the whole-frame view of the scaled views
            sq = view_geometry(SH, H, W, (-1, -1, W, H))
            for k in INT_KEYS:
                assert got[k] == sq[k], (det, H, W, k)
            for k in FLOAT_KEYS:
                assert np.float32(got[k]).view(np.uint32) == np.float32(sq[k]).view(np.uint32), (det, H, W, k)


def test_letterbox_geometry_arguments():
    from litepi import _ffi
    lib = _ffi.load_library()
    assert "lp_letterbox_geometry" in _ffi.SYMBOLS
    nul = None
    assert lib.lp_letterbox_geometry(384, 640, 1080, 1920, nul, nul, nul, nul, nul, nul, nul) == 0   # every output may be NULL
    nw, top = C.c_int(), C.c_int()
    assert lib.lp_letterbox_geometry(384, 640, 1080, 1920, nul, nul, nul, C.byref(nw), nul, C.byref(top), nul) == 0
    assert (nw.value, top.value) == (640, 12)   # 1080p into 384 x 640: 640 x 360 of picture, 2 x 12 rows of bars
    for bad in [(0, 640, 10, 10), (384, 0, 10, 10), (384, 640, 0, 10), (384, 640, 10, -1), (-32, 640, 10, 10)]:
        assert lib.lp_letterbox_geometry(*bad, nul, nul, nul, nul, nul, nul, nul) == _ffi.LP_ERR_ARG, bad
        assert b"bad argument" in lib.lp_last_error()


# sha256 of the files export_detector(preset, seed=77, size=640) wrote BEFORE sizes could be (rows, columns): (param, bin)
PARENT_SHA = {
    "v1": ("52b44c61dcae83ad94a99908aac7231385aa55a440957f718fdb0548a207edca", "99230149aab90771e580d65fb9391f3d69374e5cc9bfc8706d78bff7af6d05d8"),
    "v2": ("327f53440c191e082bb418e88a98c9d04656a5528b678cf2e0cff332409266eb", "d8b5eff67a84744a5955ad74077cf01d161ad88b56e76c502f12c6e077097421"),
}


def _sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


@pytest.mark.parametrize("preset", ["v1", "v2"])
def test_export_square_size_writes_the_same_bytes(tmp_path, preset):
    from litepi import ncnn_export
    got = {}
    for tag, size in (("int", 640), ("pair", (640, 640))):
        p, b = str(tmp_path / f"{tag}.param"), str(tmp_path / f"{tag}.bin")
        sp = ncnn_export.export_detector(p, b, preset, seed=77, size=size)
        assert sp["num_anchors"] == 8400
        got[tag] = (_sha(p), _sha(b))
    assert got["int"] == got["pair"] == PARENT_SHA[preset]


def test_export_rectangular_detector_runs_in_the_oracle(tmp_path):
    import torch
    from litepi import ncnn_export
    from litepi.ncnn_io import read_param_layers
    from oracle import ncnn_ref
    p, b = str(tmp_path / "r.param"), str(tmp_path / "r.bin")
    sp = ncnn_export.export_detector(p, b, "v1", seed=77, size=(384, 640))
    assert sp["num_anchors"] == 5040 == 48 * 80 + 24 * 40 + 12 * 20
    pts, st = ncnn_export.make_anchors((384, 640))
    want_pts, want_st = R.anchor_table(384, 640)
    assert np.array_equal(pts, want_pts) and np.array_equal(st, want_st)
    # .. and that table is what the graph carries (MemoryData payloads, in file order: strides, then the anchor points twice)
    layers = ncnn_ref.load_model(p, b)
    mem = [l for l in read_param_layers(p) if l["type"] == "MemoryData"]
    assert [(m["params"].get(0, 0), m["params"].get(1, 0)) for m in mem] == [(5040, 0), (5040, 2), (5040, 2)]
    x = torch.from_numpy(np.random.default_rng(1).random((2, 3, 384, 640), dtype=np.float32))
    out = ncnn_ref.run_graph(layers, x)["out0"].numpy()
    assert out.shape == (2, 5, 5040)
    # the decoded centres lie around their anchors, row-major: xc / stride - anchor_x is bounded by the DFL range (reg_max - 1)
    cx, cy = out[:, 0] / want_st, out[:, 1] / want_st
    assert np.abs(cx - want_pts[0]).max() <= 7.5 + 1e-3 and np.abs(cy - want_pts[1]).max() <= 7.5 + 1e-3
    # a portrait size orders its grid the same way
    pp, ps = ncnn_export.make_anchors((640, 384))
    wp, ws = R.anchor_table(640, 384)
    assert np.array_equal(pp, wp) and np.array_equal(ps, ws) and pp.shape == (2, 5040)
    assert ncnn_export.make_anchors(640)[0].shape == (2, 8400)


def test_reference_letterbox_restatement():
    """tests/rect_ref.py itself: with a square shape it is oracle.postprocess_ref.letterbox byte for byte; with 384 x 640 a 720p
    frame is 640 x 360 of picture between two bars of 12 rows of 114, and an image of the input's size is left alone"""
    from oracle import postprocess_ref as P
    rng = np.random.default_rng(3)
    for hw in [(480, 640), (640, 360), (100, 37), (640, 640)]:
        img = rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
        got, r, pad = R.letterbox(img, 640, 640)
        want, wr, wpad = P.letterbox(img, 640)
        assert np.array_equal(got, want) and r == wr and pad == wpad, hw
    img = rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    got, r, (dw, dh) = R.letterbox(img, 384, 640)
    assert got.shape == (384, 640, 3) and (r, dw, dh) == (0.5, 0.0, 12.0)
    assert (got[:12] == 114).all() and (got[372:] == 114).all()
    assert np.array_equal(got[12:372], P.resize_linear_u8(img, 640, 360))
    same = rng.integers(0, 256, (384, 640, 3), dtype=np.uint8)
    assert np.array_equal(R.letterbox(same, 384, 640)[0], same)
    tall, r, (dw, dh) = R.letterbox(rng.integers(0, 256, (1280, 720, 3), dtype=np.uint8), 640, 384)   # portrait into portrait
    assert tall.shape == (640, 384, 3) and (r, dw, dh) == (0.5, 12.0, 0.0) and (tall[:, :12] == 114).all() and (tall[:, 372:] == 114).all()


def test_reference_detect_on_a_rectangular_export(tmp_path):
    """letterbox -> graph -> postprocess at 384 x 640: the boxes come back in the frame's own pixels"""
    from litepi import ncnn_export
    from oracle import ncnn_ref
    p, b = str(tmp_path / "r.param"), str(tmp_path / "r.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, size=(384, 640), cls_bias=0.0)
    layers = ncnn_ref.load_model(p, b)
    img = np.random.default_rng(5).integers(0, 256, (720, 1280, 3), dtype=np.uint8)
    lb, _, _ = R.letterbox(img, 384, 640)
    s = np.sort(R.out0(layers, lb[None])[0, 4].astype(np.float64))[::-1]
    conf = float(0.5 * (s[11] + s[12]))   # twelve anchors pass
    boxes, scores, classes = R.detect(layers, img, 384, 640, conf, 0.45)
    assert 1 <= len(boxes) <= 12 and (scores > conf).all() and (classes == 0).all()
    assert boxes.min() >= 0 and boxes[:, [0, 2]].max() <= 1280 and boxes[:, [1, 3]].max() <= 720
    assert (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all()
