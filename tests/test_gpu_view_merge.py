"""GPU tests of the frame NMS of views with a match metric and a box-union merge (lp_set_view_merge; include/litepi.h "frame
NMS of views") against the NumPy statement of the rule (tests/view_merge_ref.py): the kernel alone through lp_test_nms_views,
bit for bit, then the three view families end to end, host against device, and the captured steps across a change of the
setting.  Models are the seeded synthetic files of tests/test_gpu_tiling.py and tests/test_gpu_views.py."""
import itertools
import os

import numpy as np
import pytest
import torch

import tiling_ref as T
import view_merge_ref as VM
from test_gpu_focus import Dev, _mixed_states, run_focus, same_frame, variants
from test_gpu_tiling import _calibrate_on_views, _random_views
from test_gpu_tiling_scenes import _REAL, _box_iou, _sign_scene
from test_gpu_views import CONF, E2E_VIEWS, H, IOU, MIN_AREA, W, _engine as _engine320, make_models

pytestmark = pytest.mark.gpu

METRICS = {"iou": VM.IOU, "ios": VM.IOS}
MODES = {"nms": VM.SUPPRESS, "union": VM.UNION}
COMBOS = list(itertools.product(METRICS, MODES))
FRAME = (2048, 2048)


@pytest.fixture(scope="module")
def eng32():
    from litepi import Engine
    e = Engine(precision="fp32", max_batch=1, max_det=300, num_classes=91)
    yield e
    e.close()


def _check(eng, cand, n_views, match, merge, max_det=None, iou=0.45, threshold=0.0, min_area=-1, frame=FRAME, ref_iou=None):
    """lp_test_nms_views under (match, merge, threshold) against the ref: boxes, scores and classes as bit patterns.  Returns the
    ref's (keepers, emitted boxes) and the records."""
    b, s, c, v, a = cand
    eng.set_view_merge(match, merge, threshold)
    try:
        dets, rects, num = eng.test_nms_views(b, s, c, v, a, n_views, frame, iou, min_area, max_det or 0)
    finally:
        eng.set_view_merge()
    k, out = VM.merge(b, s, c, v, a, iou if ref_iou is None else ref_iou, max_det, METRICS[match], MODES[merge], threshold)
    assert num == len(k), f"{match}+{merge}: {num} keepers vs the ref's {len(k)}"
    if min_area < 0:
        assert len(dets) == len(k)
        got = np.stack([dets["x1"], dets["y1"], dets["x2"], dets["y2"]], 1)
        assert np.array_equal(got.view(np.uint32), out.view(np.uint32)), f"{match}+{merge}: boxes / order differ"
        assert np.array_equal(dets["det_conf"].view(np.uint32), s[k].view(np.uint32))
        assert np.array_equal(dets["det_class"], c[k])
    return k, out, dets, rects


def _grown(cand, k, out):
    return int((out != cand[0][k]).any(axis=1).sum())


# ---------------------------------------------------------------------------- 1. the kernel against the ref
SMALL = [(3, 10), (2, 32)]                  # at most 64 candidates: the one-wave path
GENERAL = [(2, 300), (5, 200), (17, 120)]   # several chunks of 64


@pytest.mark.parametrize("match,merge", COMBOS)
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("n_views,per_view", SMALL + GENERAL)
def test_combos_vs_ref(eng32, n_views, per_view, nc, match, merge):
    rng = np.random.default_rng(n_views * 10 + nc)
    cand = _random_views(rng, n_views, per_view, nc)
    assert not np.isnan(cand[0]).any() and not (np.signbit(cand[0]) & (cand[0] == 0)).any()
    k, out, _, _ = _check(eng32, cand, n_views, match, merge)
    print(f"{n_views} x {per_view}, nc {nc}, {match}+{merge}: {len(k)} keepers, {_grown(cand, k, out)} grown boxes")
    if merge == "union":
        assert _grown(cand, k, out) >= 1, "the ref grows no box: the case is vacuous"
    else:
        assert _grown(cand, k, out) == 0
    if (match, merge) == ("iou", "nms"):
        assert np.array_equal(k, T.merge(*cand, 0.45))


@pytest.mark.parametrize("match,merge", COMBOS)
@pytest.mark.parametrize("n_views,per_view", SMALL)
def test_one_wave_path_equals_general_path(eng32, monkeypatch, n_views, per_view, match, merge):
    rng = np.random.default_rng(8 + n_views)
    for nc in (1, 3):
        cand = _random_views(rng, n_views, per_view, nc)
        _, _, small, _ = _check(eng32, cand, n_views, match, merge)
        monkeypatch.setenv("LITEPI_NMS_NO_SMALL", "1")
        _, _, general, _ = _check(eng32, cand, n_views, match, merge)
        monkeypatch.delenv("LITEPI_NMS_NO_SMALL")
        assert small.tobytes() == general.tobytes()


@pytest.mark.parametrize("match", list(METRICS))
@pytest.mark.parametrize("nc", [1, 3])
def test_max_det_with_union(eng32, nc, match):
    """nc = 1: the sweep leaves once max_det keepers are found, and the keepers of that last chunk must still take what they
    absorb in the chunks behind it; nc = 3: the cut by (score, view, anchor) over complete unions."""
    rng = np.random.default_rng(5 + nc)
    cand = _random_views(rng, 5, 200, nc)
    k, out, _, _ = _check(eng32, cand, 5, match, "union", max_det=23)
    assert len(k) == 23 and _grown(cand, k, out) >= 1
    if nc == 1:   # a keeper of the chunk that fills max_det owns a candidate behind that chunk which its box needs
        pos = np.empty(len(cand[1]), np.int64)
        pos[VM.order(*cand[1:])] = np.arange(len(pos))
        _, _, owner = VM.merge(*cand, 0.45, None, METRICS[match], VM.UNION, owners=True)
        end = (pos[k[-1]] // 64 + 1) * 64
        far = 0
        for i, box in zip(k, out):
            near = cand[0][(owner == i) & (pos < end)]
            far += int(pos[i] >= end - 64 and (near[:, :2].min(0) > box[:2]).any() | (near[:, 2:].max(0) < box[2:]).any())
        assert far >= 1, "no keeper of the last chunk needs a box from beyond it: the early-exit case is vacuous"
    _check(eng32, cand, 5, match, "nms", max_det=23)


def test_first_chunk_keeper_absorbs_in_the_last_chunk(eng32):
    """one top-score box, 200 pairwise disjoint fillers with middle scores, four cut parts of the first box with the lowest
    scores: 205 candidates in four chunks, the parts in the last"""
    whole = np.array([1000, 1000, 1080, 1060], np.float32)
    parts = np.array([[1000, 1000, 1030, 1060], [1025, 1000, 1080, 1060], [1000, 1000, 1080, 1025], [990, 995, 1050, 1070]], np.float32)
    gx, gy = np.meshgrid(np.arange(20), np.arange(10))
    fill = np.stack([gx.ravel() * 50 + 3, gy.ravel() * 50 + 3, gx.ravel() * 50 + 43, gy.ravel() * 50 + 33], 1).astype(np.float32)
    assert fill[:, 2].max() < 1000 and fill[:, 3].max() < 1000   # clear of the sign
    b = np.concatenate([whole[None], fill, parts])
    s = np.concatenate([[0.99], np.linspace(0.9, 0.5, 200), [0.30, 0.29, 0.28, 0.27]]).astype(np.float32)
    n = len(b)
    view = (np.arange(n) % 3).astype(np.int32)
    o = np.argsort(view, kind="stable")
    cand = (b[o], s[o], np.zeros(n, np.int32), view[o], np.arange(n, dtype=np.int32)[o] // 3)
    for match in METRICS:
        k, out, dets, _ = _check(eng32, cand, 3, match, "union")
        grown = out[(out != cand[0][k]).any(axis=1)]
        if match == "ios":   # every part lies (almost) inside the whole box
            assert len(k) == 201 and grown.tolist() == [[990, 995, 1080, 1070]]
        else:                # IoU takes only the parts that cover enough of it: 0.6875 and 0.476, not 0.375 and 0.417
            assert len(k) == 203 and grown.tolist() == [[990, 995, 1080, 1070]]
        assert dets["det_conf"][0] == np.float32(0.99)


def test_min_area_follows_the_merged_box(eng32):
    """two parts of 40 x 30 = 1200 pixels each, min_area 1500: apart they are both dropped, merged they pass as one 60 x 30 box"""
    b = np.array([[100.5, 200.25, 140.5, 230.25], [120.5, 200.25, 160.5, 230.25], [500, 500, 560, 540]], np.float32)
    cand = (b, np.array([0.9, 0.8, 0.7], np.float32), np.zeros(3, np.int32), np.array([0, 1, 1], np.int32), np.array([7, 7, 9], np.int32))
    k, out, dets, rects = _check(eng32, cand, 2, "ios", "union", min_area=1500)
    assert k.tolist() == [0, 2] and out[0].tolist() == [100.5, 200.25, 160.5, 230.25]
    assert len(dets) == 2 and rects.tolist() == [[100, 200, 160, 230], [500, 500, 560, 540]]
    assert [dets[n][0] for n in ("x1", "y1", "x2", "y2")] == [100.5, 200.25, 160.5, 230.25] and dets["det_conf"][0] == np.float32(0.9)
    k, _, dets, rects = _check(eng32, cand, 2, "ios", "nms", min_area=1500)
    assert k.tolist() == [0, 2] and len(dets) == 1 and rects.tolist() == [[500, 500, 560, 540]]
    k, _, dets, rects = _check(eng32, cand, 2, "iou", "nms", min_area=1500)   # IoU 1/3: today's duplicate, both below min_area
    assert k.tolist() == [0, 1, 2] and len(dets) == 1


def test_configured_threshold(eng32):
    rng = np.random.default_rng(77)
    cand = _random_views(rng, 5, 200, 3)
    for match in METRICS:
        k3, _, _, _ = _check(eng32, cand, 5, match, "union", iou=0.45, threshold=0.3, ref_iou=0.9)    # the threshold, not the iou
        k0, _, _, _ = _check(eng32, cand, 5, match, "union", iou=0.3, threshold=0.0, ref_iou=0.3)     # 0: the call's iou
        k6, _, _, _ = _check(eng32, cand, 5, match, "union", iou=0.3, threshold=0.6, ref_iou=0.3)
        assert np.array_equal(k3, k0) and len(k6) > len(k3), "the two thresholds keep the same boxes: the case is vacuous"


# ---------------------------------------------------------------------------- 2. tiled inference end to end, fp32
@pytest.fixture(scope="module")
def tiling_models(tmp_path_factory):
    """the models and scene of tests/test_gpu_tiling.py"""
    from litepi import ncnn_export, synth
    from oracle import shufflenet_ref
    d = tmp_path_factory.mktemp("view_merge_tiling")
    p, b = str(d / "m.param"), str(d / "m.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    big = synth.config4_images(1, seed=5, size=2048, grain=8)[0]
    mid = synth.config4_images(1, seed=6, size=1280, grain=8)[0][:1024]
    _calibrate_on_views(p, b, [big, mid], 4, 8)
    sd = shufflenet_ref.seeded_state_dict(91)
    cls_path = str(d / "cls.pth")
    torch.save(sd, cls_path)
    return dict(param=p, bin=b, cls=cls_path, sd=sd, big=big, mid=mid)


def test_tiled_fp32_end_to_end_ios_union_vs_oracle(tiling_models):
    from litepi import HybridPipeline
    from oracle import ncnn_ref, postprocess_ref as P, shufflenet_ref
    models = tiling_models
    frames = [models["mid"], models["big"]]
    cls = shufflenet_ref.build(91, models["sd"])
    cpu = T.CpuTiledPipeline(ncnn_ref.load_model(models["param"], models["bin"]), cls)
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, precision="fp32",
                          max_batch=34, max_det=300, tile_overlap=128, tile_full_frame=True, view_match="ios", view_merge="union")
    try:
        outs = pipe.run_batch(frames, 0.25, 0.45, 50)
    finally:
        pipe.engine.close()
    total = grown = fewer = 0
    for i, f in enumerate(frames):
        b, s, c, v, a = cpu.candidates(f, 0.25, 128, True)
        k, boxes = VM.merge(b, s, c, v, a, 0.45, None, VM.IOS, VM.UNION)
        grown += _grown((b,), k, boxes)
        fewer += len(T.merge(b, s, c, v, a, 0.45)) - len(k)
        h, w = f.shape[:2]
        rects, valid = P.roi_rects(boxes, h, w, 50)
        rois = [f[y1:y2, x1:x2] for x1, y1, x2, y2 in rects]
        ids = shufflenet_ref.predict_batch(cls, rois, 64)[0] if rois else []
        eb, es, ec = boxes[valid], s[k][valid], c[k][valid]
        res, met = outs[i]
        assert met.num_detections == len(k), f"frame {i}: num_det {met.num_detections} vs oracle {len(k)}"
        assert len(res) == len(eb), f"frame {i}: {len(res)} results vs oracle {len(eb)}"
        for n, r in enumerate(res):
            assert abs(r["det_conf"] - float(es[n])) <= 1e-3
            assert np.abs(np.array(r["bbox"]) - eb[n].astype(int)).max() <= 1
            assert r["det_class"] == int(ec[n]) and r["cls_class"] == int(ids[n])
        total += len(res)
    print(f"IoS + union on the tiled scene: {total} results, {grown} grown boxes, {fewer} boxes fewer than IoU + suppress")
    assert total >= 4, "calibration produced too few detections for a meaningful test"


# ---------------------------------------------------------------------------- 3. host and device calls, captured steps
def _engine640(models, prec, max_batch):
    from litepi import Engine
    from litepi.backend import random_shufflenet_state
    e = Engine(precision=prec, max_batch=max_batch, max_det=300, num_classes=91)
    e.load_detector(models["param"], models["bin"])
    e.load_classifier(random_shufflenet_state(91, seed=3))
    return e


def _device_result(e, B, call):
    from litepi._ffi import DET_DTYPE
    dd = torch.zeros(B * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    call(dd.data_ptr(), dc.data_ptr())
    e.synchronize()
    return dd.cpu().numpy().view(DET_DTYPE).reshape(B, -1), dc.cpu().numpy()


def _same_as_host(dev, host, avg, B, tag):
    recs, cnt = dev
    d, c, nd = host
    assert np.array_equal(cnt[:B], c) and np.array_equal(cnt[B:2 * B], nd), tag
    assert np.array_equal(cnt[2 * B:].view(np.uint32), avg.view(np.uint32)), tag
    for i in range(B):
        assert recs[i, :c[i]].tobytes() == d[i, :c[i]].tobytes(), f"{tag} frame {i}"


def _kept_bytes(dev, B):
    recs, cnt = dev
    return cnt.tobytes() + b"".join(recs[i, :cnt[i]].tobytes() for i in range(B))


def test_tiled_host_and_device_agree_and_follow_the_setting(tiling_models):
    """host call = device call under IoS + union (eager, captured, replayed); a captured default step is not replayed after the
    setting changed; after lp_set_view_merge(NULL) the records are the first call's; a handle that set and reset the merge
    equals one that never touched it"""
    models = tiling_models
    frames = np.stack([models["big"], np.ascontiguousarray(models["big"][:, ::-1])])
    B = 2
    e, fresh = _engine640(models, "fp16", 34), _engine640(models, "fp16", 34)
    try:
        buf = torch.from_numpy(frames).cuda()
        run = lambda eng: _device_result(eng, B, lambda dd, dc: eng.run_tiled_device(buf.data_ptr(), B, 2048, 2048, 0.25, 0.45, 50, dd, dc))
        first = [run(e) for _ in range(3)]   # default: eager, captured, replayed
        assert len({_kept_bytes(r, B) for r in first}) == 1
        e.set_view_merge("ios", "union")
        d, c, nd, _ = e.run_tiled(list(frames), 0.25, 0.45, 50)
        avg = e.last_det_conf_avg.copy()
        for call in range(3):
            got = run(e)
            _same_as_host(got, (d, c, nd), avg, B, f"ios+union call {call}")
        assert _kept_bytes(got, B) != _kept_bytes(first[0], B), "IoS + union changes nothing on this scene: the test is vacuous"
        assert int(nd.sum()) >= 1 and int(nd.sum()) <= int(first[0][1][B:2 * B].sum())
        from litepi._ffi import check
        check(e.lib, e.lib.lp_set_view_merge(e._h, None))
        for call in range(3):
            assert _kept_bytes(run(e), B) == _kept_bytes(first[0], B), f"after the reset, call {call}"
        assert _kept_bytes(run(fresh), B) == _kept_bytes(first[0], B), "a handle that never set the merge differs"
    finally:
        e.close()
        fresh.close()


@pytest.fixture(scope="module")
def models320(tmp_path_factory):
    return make_models(tmp_path_factory.mktemp("view_merge_views"))


def test_views_host_and_device_agree(models320):
    frames = [models320["frames"][0], models320["frames"][1]]
    B = 2
    e = _engine320(models320, "fp16", 16)
    try:
        buf = torch.from_numpy(np.stack(frames)).cuda()
        run = lambda: _device_result(e, B, lambda dd, dc: e.run_views_device(buf.data_ptr(), B, H, W, E2E_VIEWS, CONF, IOU, MIN_AREA, dd, dc))
        default = run()
        e.set_view_merge("ios", "union")
        d, c, nd, _ = e.run_views(frames, E2E_VIEWS, CONF, IOU, MIN_AREA)
        avg = e.last_det_conf_avg.copy()
        for call in range(3):
            got = run()
            _same_as_host(got, (d, c, nd), avg, B, f"views call {call}")
        assert int(nd.sum()) >= 1
        print(f"views: {int(default[1][B:2 * B].sum())} keepers by default, {int(nd.sum())} under IoS + union")
    finally:
        e.close()


def test_focus_host_and_device_agree(models320):
    frames = variants(models320)
    e = _engine320(models320, "fp16", 12)
    try:
        e.set_view_merge("ios", "union")
        _mixed_states(e)
        dev = Dev(e, frames, 3)
        for call in range(3):
            d, c, nd, _, views = e.run_focus(frames, CONF, IOU, MIN_AREA, stream_ids=[0, 1, 2])
            avg = e.last_det_conf_avg.copy()
            got = run_focus(e, dev, [0, 1, 2])
            assert np.array_equal(views, got[2])
            host = (d, np.concatenate([c.astype(np.int32), nd.astype(np.int32), avg.view(np.int32)]))
            for i in range(3):
                same_frame(got, i, 3, host, i, 3, f"focus call {call} frame {i}")
    finally:
        e.close()


# ---------------------------------------------------------------------------- 4. real v1 weights: a sign across a tile border
@pytest.mark.skipif(not all(os.path.exists(p) for p in _REAL), reason="the reference's v1 model is not staged under oracle/_ref")
def test_real_v1_weights_sign_across_a_tile_border(tmp_path):
    """The sign scene of tests/test_gpu_tiling_scenes.py with its largest sign pasted once more across x = 640, the right edge of
    the first tile column at overlap 0 and at overlap 128.  A statement about the model: printed, not asserted."""
    from litepi import HybridPipeline
    from oracle import shufflenet_ref as S
    img, rects = _sign_scene()
    k = int(np.argmax([(r[2] - r[0]) * (r[3] - r[1]) for r in rects]))
    x1, y1, x2, y2 = rects[k]
    w, h = x2 - x1, y2 - y1
    bx, by = 640 - w // 2, 450
    img[by:by + h, bx:bx + w] = img[y1:y2, x1:x2]
    border = (bx, by, bx + w, by + h)
    rects = rects + [border]
    cls_path = str(tmp_path / "cls.pth")
    torch.save(S.seeded_state_dict(58), cls_path)
    lines = []
    for overlap in (0, 128):
        for name, kw in (("default", {}), ("IoS + union", dict(view_match="ios", view_merge="union"))):
            pipe = HybridPipeline(*_REAL, cls_path, "shufflenetv2", num_classes=58, precision="fp32", max_batch=17, max_det=8400,
                                  max_rois=8400, tile_overlap=overlap, **kw)
            try:
                res, met = pipe.run_batch([img], 0.25, 0.45, 50)[0]
            finally:
                pipe.engine.close()
            boxes = [np.array(r["bbox"], np.float64) for r in res]
            found = sum(any(_box_iou(np.array(rc, np.float64), b) >= 0.5 for b in boxes) for rc in rects)
            on_border = sum(1 for b in boxes if _box_iou(np.array(border, np.float64), b) > 0 and
                            (min(b[2], border[2]) - max(b[0], border[0])) * (min(b[3], border[3]) - max(b[1], border[1])) >=
                            0.5 * (b[2] - b[0]) * (b[3] - b[1]))
            hit = any(_box_iou(np.array(border, np.float64), b) >= 0.5 for b in boxes)
            lines.append(f"overlap {overlap:3d}, {name:11s}: {len(res)} kept boxes ({met.num_detections} before min_area), {found} of "
                         f"{len(rects)} signs found, {on_border} boxes on the border sign ({w}x{h} px), found: {hit}")
    print("\n[view merge] real v1 weights, 2048x2048 sign scene + one sign across the tile border x = 640, conf 0.25, IoU >= 0.5:\n  " +
          "\n  ".join(lines))
