"""GPU tests of tiled inference (lp_run_tiled, lp_run_tiled_device, the frame NMS through lp_test_nms_views) against the
host path lp_run_batch and the CPU tiling oracle (tests/tiling_ref.py).  Models are seeded synthetic files."""
import numpy as np
import pytest
import torch

import tiling_ref as T

pytestmark = pytest.mark.gpu


def _calibrate_on_views(param, binf, frames, lo, hi):
    """shift the class biases so that between lo and hi candidates per view pass conf 0.25, with the threshold in the widest
    gap between two neighbouring scores of that range (no candidate sits within 1e-3 of it, so fp32 and the oracle agree on
    the filter)"""
    from litepi import ncnn_export
    from oracle import ncnn_ref, postprocess_ref as P
    layers = ncnn_ref.load_model(param, binf)
    views = [v for f in frames for v, _, _ in T.make_views(f, 640, 128, True)]
    outs = []
    with torch.no_grad():
        for i in range(0, len(views), 8):
            x = np.concatenate([P.preprocess(v, 640)[0] for v in views[i:i + 8]])
            outs.append(ncnn_ref.run_graph(layers, torch.from_numpy(x))["out0"].numpy())
    s = np.sort(np.concatenate(outs)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    ks = np.arange(lo * len(views), hi * len(views))
    k = int(ks[np.argmax(np.log(s[ks - 1] / (1 - s[ks - 1])) - np.log(s[ks] / (1 - s[ks])))])
    logit = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(param, binf, float(np.log(0.25 / 0.75) - logit))


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from litepi import ncnn_export, synth
    from oracle import shufflenet_ref
    d = tmp_path_factory.mktemp("tiling")
    p, b = str(d / "m.param"), str(d / "m.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    big = synth.config4_images(1, seed=5, size=2048, grain=8)[0]
    mid = synth.config4_images(1, seed=6, size=1280, grain=8)[0][:1024]
    _calibrate_on_views(p, b, [big, mid], 4, 8)
    sd = shufflenet_ref.seeded_state_dict(91)
    cls_path = str(d / "cls.pth")
    torch.save(sd, cls_path)
    return dict(param=p, bin=b, cls=cls_path, sd=sd, big=big, mid=mid)


def _engine(models, prec, max_batch, classifier=True, max_det=300, max_rois=0):
    from litepi import Engine
    from litepi.backend import random_shufflenet_state
    e = Engine(precision=prec, max_batch=max_batch, max_det=max_det, num_classes=91, max_rois=max_rois)
    e.load_detector(models["param"], models["bin"])
    if classifier:
        e.load_classifier(random_shufflenet_state(91, seed=3))
    return e


# ---------------------------------------------------------------------------- 1. frames that fit one tile
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_one_tile_frames_equal_run_batch(models, prec):
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (640, 640, 3), dtype=np.uint8), models["big"][100:500, 300:800].copy()]
    e = _engine(models, prec, 4)
    try:
        ref = e.run_batch(frames, 0.25, 0.45, 50)
        ref_avg = e.last_det_conf_avg.copy()
        for _ in range(3):   # eager, captured, replayed
            got = e.run_tiled(frames, 0.25, 0.45, 50, overlap=128, full_frame=True)
            assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
            assert np.array_equal(e.last_det_conf_avg.view(np.uint32), ref_avg.view(np.uint32))
            for i in range(2):
                n = int(ref[1][i])
                assert got[0][i, :n].tobytes() == ref[0][i, :n].tobytes(), f"frame {i}: records differ"
        assert int(ref[2].sum()) >= 1, "the calibrated model found nothing: the comparison is empty"
    finally:
        e.close()


# ---------------------------------------------------------------------------- 2. the frame NMS against the oracle merge
def _random_views(rng, n_views, per_view, nc, H=2048, W=2048, ties=True):
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


def _check_nms_views(eng, b, s, c, v, a, n_views, max_det=None, H=2048, W=2048):
    k = T.merge(b, s, c, v, a, 0.45, max_det)
    dets, _, num = eng.test_nms_views(b, s, c, v, a, n_views, (H, W), 0.45, -1, max_det or 0)
    assert num == len(k) == len(dets), f"kept {len(dets)} (pre-filter {num}) vs oracle {len(k)}"
    got = np.stack([dets["x1"], dets["y1"], dets["x2"], dets["y2"]], 1)
    assert np.array_equal(got.view(np.uint32), b[k].view(np.uint32)), "boxes / order differ"
    assert np.array_equal(dets["det_conf"].view(np.uint32), s[k].view(np.uint32))
    assert np.array_equal(dets["det_class"], c[k])


@pytest.fixture(scope="module")
def eng32(models):
    from litepi import Engine
    e = Engine(precision="fp32", max_batch=1, max_det=300, num_classes=91)
    yield e
    e.close()


@pytest.mark.parametrize("n_views,per_view", [(2, 300), (5, 200), (17, 120)])
@pytest.mark.parametrize("nc", [1, 3])
def test_nms_views_vs_oracle(eng32, n_views, per_view, nc):
    rng = np.random.default_rng(n_views * 10 + nc)
    _check_nms_views(eng32, *_random_views(rng, n_views, per_view, nc), n_views)


def test_nms_views_cross_view_exact_ties(eng32):
    # the same box and score from three views and two anchors: the highest (view, anchor) is the one kept
    b = np.array([[600, 100, 640, 140]] * 4, np.float32)
    s = np.full(4, 0.5, np.float32)
    c = np.zeros(4, np.int32)
    v = np.array([0, 1, 2, 2], np.int32)
    a = np.array([9000 - 1, 17, 3, 4], np.int32)
    _check_nms_views(eng32, b, s, c, v, a, 3)


@pytest.mark.parametrize("nc", [1, 3])
def test_nms_views_max_det_cuts_union(eng32, nc):
    rng = np.random.default_rng(5 + nc)
    _check_nms_views(eng32, *_random_views(rng, 5, 200, nc), 5, max_det=23)


def test_nms_views_one_wave_path_equals_general(eng32, monkeypatch):
    rng = np.random.default_rng(8)
    for n_views, per in [(3, 10), (17, 3), (2, 32)]:   # 30, 51, 64 candidates
        args = _random_views(rng, n_views, per, 2)
        _check_nms_views(eng32, *args, n_views)
        monkeypatch.setenv("LITEPI_NMS_NO_SMALL", "1")
        _check_nms_views(eng32, *args, n_views)
        monkeypatch.delenv("LITEPI_NMS_NO_SMALL")


def test_nms_views_union_beyond_one_lds_sort(eng32):
    # 3 x 6000 = 18000 candidates: more than the 16384 keys one workgroup sorts in LDS; exact all the same
    rng = np.random.default_rng(21)
    b, s, c, v, a = _random_views(rng, 3, 6000, 3, ties=True)
    assert len(s) > 16384
    _check_nms_views(eng32, b, s, c, v, a, 3)


def _one_view_candidates(n, nc, seed):
    """n clustered candidates of one view with exact score ties, anchors = their indices; every seventh box is a few pixels
    small, so that min_area 50 drops some and passes others"""
    rng = np.random.default_rng(seed)
    b, s, c, v, _ = _random_views(rng, 1, n, nc)
    small = np.arange(3, n, 7)
    b[small, 2:] = b[small, :2] + rng.uniform(3, 9, (len(small), 2)).astype(np.float32)
    return b, s, c, v, np.arange(n, dtype=np.int32)


def _same_from_both_hooks(eng, cand, max_det, min_area, H=2048, W=2048):
    """the image NMS (test_nms_boxes) and the frame NMS of ONE view (test_nms_views) on the same list: byte-equal records,
    rects and counts, and both equal to the oracle (per-class reference NMS, its tie rule, then the ROI rule)"""
    from oracle import postprocess_ref as P
    b, s, c, v, a = cand
    img = eng.test_nms_boxes(b, s, c, (H, W), 0.45, min_area, max_det or 0)
    frm = eng.test_nms_views(b, s, c, v, a, 1, (H, W), 0.45, min_area, max_det or 0)
    assert img[2] == frm[2] and len(img[0]) == len(frm[0])
    assert img[0].tobytes() == frm[0].tobytes(), "records differ between the image NMS and the one-view frame NMS"
    assert np.array_equal(img[1], frm[1])
    k = T.merge(b, s, c, v, a, 0.45, max_det)
    assert img[2] == len(k)
    rects, valid = P.roi_rects(b[k], H, W, min_area)
    kv = k[valid]
    d = img[0]
    assert len(d) == len(kv)
    got = np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], 1) if len(d) else np.zeros((0, 4), np.float32)
    assert np.array_equal(got.view(np.uint32), b[kv].view(np.uint32)), "boxes / order differ from the oracle"
    assert np.array_equal(d["det_conf"].view(np.uint32), s[kv].view(np.uint32)) and np.array_equal(d["det_class"], c[kv])
    assert np.array_equal(img[1], rects)
    return len(k), len(kv)


@pytest.mark.parametrize("nc", [1, 3])
def test_one_view_frame_nms_is_the_image_nms(eng32, monkeypatch, nc):
    """the image NMS is the one-view case of the frame NMS: one core (nms_dev.h) behind both hooks.  Counts around the one-wave
    limit and the chunk size; max_det 0 (keep all) and a max_det below the survivors (nc 1: the sweep's early exit, nc 3: the
    threshold-key cut); counts <= 64 also with the one-wave path switched off."""
    dropped = 0
    for n in (0, 1, 64, 65, 128, 129, 200, 700):
        cand = _one_view_candidates(n, nc, 100 * nc + n)
        nk, nv = _same_from_both_hooks(eng32, cand, None, 50)
        dropped += nk - nv
        cuts = [None] + ([max(1, nk // 2)] if nk >= 2 else [])   # (0 or 1 survivors: no max_det lies below them)
        for max_det in cuts[1:]:
            assert _same_from_both_hooks(eng32, cand, max_det, 50)[0] == max_det
        if n <= 64:
            monkeypatch.setenv("LITEPI_NMS_NO_SMALL", "1")
            try:
                for max_det in cuts:
                    _same_from_both_hooks(eng32, cand, max_det, 50)
            finally:
                monkeypatch.delenv("LITEPI_NMS_NO_SMALL")
    assert dropped >= 1, "min_area dropped nothing: the filter is not exercised"


def _chunk_clusters(n, seed):
    """n candidates of two classes with distinct scores, view-major over three views: n // 8 disjoint cluster heads hold the top
    scores, every other box is a jittered copy of a random head with a lower score.  In the sweep's order the heads come first
    in their class and take members from every later chunk of 64; members that escape their head become keepers further back.
    Class 0 is a quarter of the clusters, so class 1's heads still lie in the first chunk and its members reach to the end."""
    rng = np.random.default_rng(seed)
    nh = max(2, n // 8)
    gx, gy = np.divmod(np.arange(nh), 6)
    heads = np.stack([gx * 70 + 10, gy * 70 + 10, gx * 70 + 50, gy * 70 + 50], 1).astype(np.float32)
    of = rng.integers(0, nh, n - nh)
    jit = rng.normal(0, 5, (n - nh, 4)).astype(np.float32)
    b = np.concatenate([heads, heads[of] + jit]).clip(0, 2048).astype(np.float32)
    c = np.concatenate([np.arange(nh) % 4 != 0, of % 4 != 0]).astype(np.int32)
    s = np.linspace(0.99, 0.30, n).astype(np.float32)
    s[nh:] = s[nh:][rng.permutation(n - nh)]
    p = rng.permutation(n)   # candidate order says nothing about the score
    b, s, c = b[p], s[p], c[p]
    v = np.sort(np.arange(n) % 3).astype(np.int32)
    a = np.concatenate([np.arange((v == k).sum()) for k in range(3)]).astype(np.int32)
    return b, s, c, v, a


def _cross_chunk(cand, metric):
    """from the oracle alone: the largest distance, in chunks of 64 of the sweep's order, between an absorbed box and its keeper"""
    import view_merge_ref as VM
    pos = np.empty(len(cand[1]), np.int64)
    pos[VM.order(*cand[1:])] = np.arange(len(pos))
    _, _, owner = VM.merge(*cand, 0.45, None, metric, VM.SUPPRESS, owners=True)
    return int((pos // 64 - pos[owner] // 64).max())


@pytest.mark.parametrize("n", [65, 127, 128, 129, 193])
def test_nms_chunk_boundaries(eng32, n):
    """a keeper of chunk k suppresses (and, under union, absorbs) boxes of chunks k + 1 and, where the list has a third chunk,
    k + 2: the outer phase of the sweep.  The image kernel against the reference's NMS, the frame kernel under all four
    (match, merge) settings against view_merge_ref."""
    import view_merge_ref as VM
    from oracle import postprocess_ref as P
    cand = _chunk_clusters(n, 40 + n)
    b, s, c, v, a = cand
    assert len(np.unique(s)) == n
    reach = min(2, (n - 1) // 64)
    for metric in (VM.IOU, VM.IOS):
        assert _cross_chunk(cand, metric) >= reach, "no keeper reaches that far: the case is vacuous"
    # the image kernel: one view, anchors = indices; the scores are distinct, so the order is the same
    k = T.merge(b, s, c, np.zeros(n, np.int32), np.arange(n), 0.45)
    assert np.array_equal(k, T.merge(b, s, c, v, a, 0.45)) and 2 <= len(k) < n
    d, _, num = eng32.test_nms_boxes(b, s, c, (2048, 2048), 0.45, -1, 0)
    assert num == len(k) == len(d)
    assert np.array_equal(np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], 1).view(np.uint32), b[k].view(np.uint32))
    assert np.array_equal(d["det_conf"].view(np.uint32), s[k].view(np.uint32)) and np.array_equal(d["det_class"], c[k])
    _check_nms_views(eng32, b, s, c, v, a, 3)
    for match, metric in (("iou", VM.IOU), ("ios", VM.IOS)):
        for merge, mode in (("nms", VM.SUPPRESS), ("union", VM.UNION)):
            eng32.set_view_merge(match, merge, 0.0)
            try:
                d, _, num = eng32.test_nms_views(b, s, c, v, a, 3, (2048, 2048), 0.45, -1, 0)
            finally:
                eng32.set_view_merge()
            kk, out = VM.merge(b, s, c, v, a, 0.45, None, metric, mode)
            assert num == len(kk) == len(d), f"{match}+{merge}"
            assert np.array_equal(np.stack([d["x1"], d["y1"], d["x2"], d["y2"]], 1).view(np.uint32), out.view(np.uint32)), f"{match}+{merge}"
            assert np.array_equal(d["det_conf"].view(np.uint32), s[kk].view(np.uint32)) and np.array_equal(d["det_class"], c[kk])
            if mode == VM.UNION:   # a grown box whose absorbed boxes lie in a later chunk than the keeper
                pos = np.empty(n, np.int64)
                pos[VM.order(s, c, v, a)] = np.arange(n)
                owner = VM.merge(b, s, c, v, a, 0.45, None, metric, mode, owners=True)[2]
                far = [i for i, o in zip(kk, out) if (o != b[i]).any() and (pos[owner == i] // 64 > pos[i] // 64).any()]
                assert far, f"{match}+union: no union reaches into a later chunk"


# ---------------------------------------------------------------------------- 3. fp32 end to end against the tiling oracle
@pytest.mark.parametrize("full_frame", [1, 0])
def test_tiled_fp32_end_to_end_vs_oracle(models, full_frame):
    from litepi import HybridPipeline
    from oracle import ncnn_ref, shufflenet_ref
    frames = [models["mid"], models["big"]]
    cpu = T.CpuTiledPipeline(ncnn_ref.load_model(models["param"], models["bin"]), shufflenet_ref.build(91, models["sd"]))
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, precision="fp32",
                          max_batch=34, max_det=300, tile_overlap=128, tile_full_frame=bool(full_frame))
    try:
        outs = pipe.run_batch(frames, 0.25, 0.45, 50)
    finally:
        pipe.engine.close()
    total = 0
    for i, f in enumerate(frames):
        exp, exp_num = cpu.run(f, 0.25, 0.45, 50, overlap=128, full_frame=bool(full_frame))
        res, met = outs[i]
        assert met.num_detections == exp_num, f"frame {i}: num_det {met.num_detections} vs oracle {exp_num}"
        assert len(res) == len(exp), f"frame {i}: {len(res)} results vs oracle {len(exp)}"
        for r, x in zip(res, exp):
            assert abs(r["det_conf"] - x["det_conf"]) <= 1e-3
            assert np.abs(np.array(r["bbox"]) - np.array(x["bbox"])).max() <= 1
            assert r["det_class"] == x["det_class"] and r["cls_class"] == x["cls_class"]
        total += len(res)
    assert total >= 4, "calibration produced too few detections for a meaningful test"


# ---------------------------------------------------------------------------- 5. device path
def test_tiled_device_path_equals_host_path(models):
    from litepi._ffi import DET_DTYPE
    e = _engine(models, "fp16", 34)
    try:
        frames = np.stack([models["big"], np.ascontiguousarray(models["big"][:, ::-1])])
        B = 2
        dets_ref, counts_ref, num_ref, _ = e.run_tiled(list(frames), 0.25, 0.45, 50)
        avg_ref = e.last_det_conf_avg.copy()
        bufs = [torch.from_numpy(frames).cuda(), torch.from_numpy(frames.copy()).cuda()]
        dd = torch.zeros(B * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for call in range(5):   # eager, capturing, replayed ..., two alternating input buffers
            e.run_tiled_device(bufs[call % 2].data_ptr(), B, 2048, 2048, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            cnt = dc.cpu().numpy()
            assert np.array_equal(cnt[:B], counts_ref) and np.array_equal(cnt[B:2 * B], num_ref), f"call {call}"
            assert np.array_equal(cnt[2 * B:].view(np.uint32), avg_ref.view(np.uint32)), f"call {call}"
            recs = dd.cpu().numpy().view(DET_DTYPE).reshape(B, -1)
            for i in range(B):
                assert recs[i, :counts_ref[i]].tobytes() == dets_ref[i, :counts_ref[i]].tobytes(), f"call {call} frame {i}"
        assert int(num_ref.sum()) >= 1
    finally:
        e.close()


# ---------------------------------------------------------------------------- 6. errors
def test_tiled_errors(models):
    from litepi._ffi import LP_ERR_ARG, LP_ERR_STATE, LitepiError
    big = models["big"]
    e = _engine(models, "fp16", 16)
    try:
        with pytest.raises(LitepiError) as ex:   # 17 views > max_batch 16: refused, nothing truncated
            e.run_tiled([big], 0.25, 0.45, 50, overlap=128, full_frame=True)
        assert ex.value.code == LP_ERR_ARG
        for bad in (-1, 640):
            with pytest.raises(LitepiError) as ex:
                e.run_tiled([big[:600, :600]], 0.25, 0.45, 50, overlap=bad)
            assert ex.value.code == LP_ERR_ARG
        e.run_tiled([big], 0.25, 0.45, 50, overlap=128, full_frame=False)   # 16 views fit
    finally:
        e.close()
    e = _engine(models, "fp16", 17, classifier=False)
    try:
        codes = []
        for fn in (lambda: e.run_batch([big], 0.25, 0.45, 50), lambda: e.run_tiled([big], 0.25, 0.45, 50)):
            with pytest.raises(LitepiError) as ex:
                fn()
            codes.append(ex.value.code)
        assert codes == [LP_ERR_STATE, LP_ERR_STATE]
    finally:
        e.close()


# ---------------------------------------------------------------------------- 7. the staged host pass behind lp_run_tiled
def test_tiled_host_pass_timing_and_roi_overflow(models):
    """lp_run_tiled goes through the same staged host pass as lp_run_batch (run_host_pass): the stage times come from the four
    events around the three captured pieces, and a max_rois that is too small is an error raised after the records were
    delivered, which leaves the handle usable.

    The confidence is 0.20, not the 0.25 of the other tests: the fixture calibrates 4..8 candidates per view over the 24 views
    of big and mid together, and every one of them falls on big (the fp32 oracle's best score on mid is 0.235, so at 0.25 mid
    has no record at all).  At 0.20 the oracle (CpuTiledPipeline) has 300 candidates on mid's 7 views (24..57 per view) and 179
    records after the frame NMS, 5 candidates lie above 0.2276 (more than the fp16 score bound of 0.02 over the threshold), and
    mid[:640, :640] has none at 0.25."""
    from litepi._ffi import LP_ERR_STATE, LitepiError
    mid = models["mid"]
    assert mid.shape[:2] == (1024, 1280)
    tile = np.ascontiguousarray(mid[:640, :640])
    e = _engine(models, "fp16", 8)
    try:
        assert len(e.tile_grid(1024, 1280, overlap=128, full_frame=True)) == 7
        _, counts, _, t = e.run_tiled([mid], 0.20, 0.45, 0, overlap=128, full_frame=True)
        print(f"records {int(counts.sum())}, t_detection {t.t_detection:.4f} t_roi_extract {t.t_roi_extract:.4f} "
              f"t_classification {t.t_classification:.4f} t_total {t.t_total:.4f} ms")
        assert int(counts.sum()) >= 2, "the calibrated model found fewer than 2 records: the comparison is empty"
        stages = (t.t_detection, t.t_roi_extract, t.t_classification)
        assert all(x > 0 for x in stages), stages
        assert all(t.t_total >= x for x in stages), (t.t_total, stages)   # event 0 .. event 3 encloses all three
        # a confidence at which the one-tile frame keeps at most one record, found on this (default max_rois) engine
        few = [c for c in (0.25, 0.5, 0.75, 0.9, 0.99, 1.0) if int(e.run_tiled([tile], c, 0.45, 0)[1].sum()) <= 1]
        assert few, "no confidence leaves at most one record on the one-tile frame"
    finally:
        e.close()
    e = _engine(models, "fp16", 8, max_rois=1)
    try:
        with pytest.raises(LitepiError) as ex:
            e.run_tiled([mid], 0.20, 0.45, 0, overlap=128, full_frame=True)
        assert ex.value.code == LP_ERR_STATE and "max_rois" in str(ex.value)
        _, counts, _, _ = e.run_tiled([tile], few[0], 0.45, 0, overlap=128, full_frame=True)   # the handle is still usable
        assert int(counts.sum()) <= 1
    finally:
        e.close()
