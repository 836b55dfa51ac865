"""The ROI resize dealt as (ROI, strip of 16 output rows) units: every byte against oracle.pil_resize_ref.resize_bilinear_u8
(Pillow's bilinear resize restated, itself pinned to Pillow by test_roi_resize_bit_exact_vs_pillow) on the RGB crop.

Whole crops go through test_roi_resize, which places each crop at (0, 0) of an "image" of its own on a 16-byte aligned offset;
rectangles of one frame go through test_roi_resize_rects, whose frame buffer is exactly H * W * 3 bytes: ROIs at every x residue
modulo 4, rows on all four alignments (odd frame width) and the buffer's first and last byte inside a ROI.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIDES = [1, 2, 3, 4, 5, 7, 15, 16, 17, 31, 33, 63, 64, 65, 66, 127, 128, 129, 130, 191, 193, 255, 257, 383, 384, 385, 386]
# up- and down-scaling, strip windows that overlap (in_h < 64) and abut, both identity passes, every mode boundary, the large variant
EXTRA = [(64, 64), (64, 30), (30, 64), (128, 384), (129, 384), (384, 384), (385, 385), (700, 500)]   # (h, w)


@pytest.fixture(scope="module")
def eng():
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=4, max_det=300, num_classes=91)
    yield e
    e.close()


def _expect(crop_bgr):
    from oracle import pil_resize_ref as R
    return R.resize_bilinear_u8(np.ascontiguousarray(crop_bgr[:, :, ::-1]), 64, 64)


def _check(got, crops, what):
    assert got.shape == (len(crops), 64, 64, 3)
    for i, (g, c) in enumerate(zip(got, crops)):
        exp = _expect(c)
        bad = np.argwhere(g != exp)
        assert len(bad) == 0, (f"{what} {i}, crop {c.shape[:2]}: {len(bad)} bytes differ, first at (y, x, c) = {tuple(bad[0])}, "
                               f"max diff {np.abs(g.astype(int) - exp.astype(int)).max()}")


def test_whole_crops_every_height(eng):
    rng = np.random.default_rng(11)
    crops = [rng.integers(0, 256, (h, 24, 3), dtype=np.uint8) for h in SIDES]
    _check(eng.test_roi_resize(crops), crops, "height case")


def test_whole_crops_every_width(eng):
    rng = np.random.default_rng(12)
    crops = [rng.integers(0, 256, (24, w, 3), dtype=np.uint8) for w in SIDES]
    _check(eng.test_roi_resize(crops), crops, "width case")


def test_whole_crops_mode_boundaries(eng):
    rng = np.random.default_rng(13)
    crops = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in EXTRA]
    _check(eng.test_roi_resize(crops), crops, "boundary case")


def test_large_variant_identity_passes_and_split_x_table(eng):
    """Beyond 384 pixels: each identity pass with the other side large, and a crop whose two tap tables together pass the
    workgroup's LDS, so that the x table is staged in two halves."""
    rng = np.random.default_rng(18)
    crops = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((400, 64), (64, 400), (3600, 3600))]
    _check(eng.test_roi_resize(crops), crops, "large case")


def test_more_units_than_any_grid(eng):
    """600 crops are 2400 units: every workgroup takes several, whatever the device's grid."""
    rng = np.random.default_rng(14)
    crops = [rng.integers(0, 256, (8, 8, 3), dtype=np.uint8) for _ in range(600)]
    _check(eng.test_roi_resize(crops), crops, "crop")


def _rect_crops(frame, rects):
    return [frame[y1:y2, x1:x2] for x1, y1, x2, y2 in rects]


def test_rectangles_of_an_odd_width_frame(eng):
    rng = np.random.default_rng(15)
    H, W = 97, 131   # 393 bytes per row: consecutive rows start at all four alignments
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rects = [(x, 3 + x, x + 40 + x, 3 + x + 30) for x in (4, 5, 6, 7)]          # every x residue modulo 4
    rects += [(x, 50, x + 64, 90) for x in (1, 2, 3, 8)]                        # the same through the horizontal identity pass
    rects += [(0, 0, 20, 17), (W - 21, 0, W, 19), (0, H - 18, 23, H), (W - 22, H - 20, W, H)]   # the four corners
    rects += [(0, 0, 1, 1), (W - 1, H - 1, W, H)]                               # the buffer's first and last pixel alone
    rects += [(0, 0, W, H), (77, 41, 78, 42), (0, 33, W, 34), (65, 0, 66, H)]   # whole frame, 1 x 1, one row, one column
    _check(eng.test_roi_resize_rects(frame, rects), _rect_crops(frame, rects), "rectangle")


def test_rectangles_beyond_the_banded_limits(eng):
    rng = np.random.default_rng(16)
    H, W = 300, 420
    frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    rects = [(0, 0, W, H), (1, 0, 387, 300), (33, 2, 420, 131), (7, 9, 7 + 384, 9 + 129), (2, 100, 391, 164),
             (350, 1, 414, 299), (0, 0, 419, 129), (3, 150, 420, 300)]
    _check(eng.test_roi_resize_rects(frame, rects), _rect_crops(frame, rects), "rectangle")


def test_linear_numerics_every_height():
    """numerics="e2e_optimize": the cv2-linear resize of oracle/optimize_ref.py, dealt by the same units."""
    from litepi import Engine
    from oracle import optimize_ref as O
    rng = np.random.default_rng(17)
    crops = [rng.integers(0, 256, (h, 24, 3), dtype=np.uint8) for h in SIDES]
    frame = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    rects = [(5, 3, 60, 40), (0, 0, 131, 97), (130, 96, 131, 97), (2, 1, 66, 65)]
    e = Engine(precision="fp32", max_batch=1, numerics="e2e_optimize")
    try:
        got = e.test_roi_resize(crops)
        want = O.preprocess_rois(crops, 64)
        assert got.shape == want.shape
        bad = [(c.shape[0], int((g != w).sum())) for c, g, w in zip(crops, got, want) if (g != w).any()]
        assert not bad, f"(height, differing bytes) against the cv2-linear oracle: {bad}"
        got = e.test_roi_resize_rects(frame, rects)
        want = O.preprocess_rois(_rect_crops(frame, rects), 64)
        assert np.array_equal(got, want)
    finally:
        e.close()
