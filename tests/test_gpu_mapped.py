"""GPU tests of mapped views (lp_map_add, lp_run_mapped, lp_run_mapped_device, the gather and the candidate kernel through
lp_test_map_views / lp_test_map_boxes) against the NumPy restatement of the three rules and the CPU oracle (tests/mapped_ref.py),
and against the existing paths (lp_run_views, lp_run_batch).  Models are the seeded det_input 320 files of tests/test_gpu_views.py."""
import numpy as np
import pytest
import torch

import mapped_ref as M
import tiling_ref as T
from test_gpu_views import CONF, E2E_FRAME, E2E_VIEWS, H, IOU, MIN_AREA, S, W, _engine, _same_host, make_models

pytestmark = pytest.mark.gpu

# the maps of the end-to-end tests: the frame's centre turned by 7 degrees at 1.3 frame pixels per view pixel, and a barrel map
E2E_MAPS = lambda: [M.rotated(S, H, W, 7.0, 1.3), M.barrel(S, H, W, -0.3)]   # noqa: E731
# what the fp32 oracle (CpuMappedPipeline.run_mapped on frame E2E_FRAME with ["full"] + E2E_MAPS at conf 0.25, iou 0.45,
# min_area 50) keeps after the frame NMS: 3 of the whole frame, 3 of the rotation, 5 of the barrel map; computed on the CPU
# before the first GPU run
E2E_ORACLE_KEPT = 11
# test 4: the frame (litepi.synth.config4_images seed, index) and the threshold at which no candidate of the twelve crops of the
# tile grid comes within 0.25 px of an edge of its view that is not the frame's edge (in the CPU oracle; the nearest score is
# 5e-3 from the threshold), so that decoding as a crop of an S x S image, which clips to the view, clips exactly what decoding
# as a window of the frame clips.  The oracle keeps 4 records there; CROP_SHARE: the share of them all of whose coordinates lie
# at least 2e-3 from an integer.  Found by a search over seeds 1..119, both frames, thresholds 0.25..0.5.
CROP_SEED, CROP_FRAME, CROP_CONF, CROP_SHARE = 48, 1, 0.28, 1.0


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return make_models(tmp_path_factory.mktemp("mapped"))


# ---------------------------------------------------------------------------- 1. the gather, 2. the boxes
GATHER_SHAPES = [(150, 210), (333, 517), (70, 720)]
GATHER_CASES = [(shape, s) for s in (64, 320) for shape in GATHER_SHAPES]


@pytest.fixture(scope="module")
def gather_engines():
    from litepi import Engine
    es = {s: Engine(precision="fp32", max_batch=16, max_det=8, num_classes=4, det_input=s) for s in (64, 320)}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("shape,s", GATHER_CASES, ids=[f"{sh[0]}x{sh[1]}-{s}" for sh, s in GATHER_CASES])
def test_map_gather_bytes_and_boxes_equal_numpy(gather_engines, shape, s):
    """lp_test_map_views is byte-equal to mapped_ref.render at byte offsets 0, 1, 7 and 48 (the buffer ends with the frame's last
    byte), and lp_test_map_boxes bit-equal to mapped_ref.map_box, for every map of mapped_ref.cases"""
    eng = gather_engines[s]
    Hh, Ww = shape
    img = np.random.default_rng(Hh * 7 + s).integers(0, 256, shape + (3,), dtype=np.uint8)
    maps = M.cases(s, Hh, Ww)
    eng.map_clear()
    try:
        ids = [eng.map_add(xy, Hh, Ww) for xy in maps.values()]
        assert ids == list(range(len(maps)))
        fixed = [M.fixed(xy, Hh, Ww) for xy in maps.values()]
        want = np.stack([M.render(fx, img) for fx in fixed])
        assert (want[list(maps).index("outside")] == 114).all() and want[list(maps).index("random")].std() > 20
        for off in (0, 1, 7, 48):
            got = eng.test_map_views(img, ids, byte_offset=off)
            for k, name in enumerate(maps):
                assert np.array_equal(got[k], want[k]), (f"{shape} S {s} offset {off} map {name}: {int((got[k] != want[k]).sum())} bytes "
                                                         f"differ, first at {np.argwhere(got[k] != want[k])[0].tolist()}")
        got = eng.test_map_views(img, ids[::-1] + [ids[3]], byte_offset=5)   # list order, and an id twice
        assert np.array_equal(got, want[[ids[::-1] + [ids[3]]][0]])
        boxes = M.boxes(s, seed=Hh + Ww)
        for k, name in enumerate(maps):
            wb = M.map_box(fixed[k], Hh, Ww, boxes)
            gb = eng.test_map_boxes(ids[k], boxes)
            bad = np.argwhere(gb.view(np.uint32) != wb.view(np.uint32))
            assert bad.size == 0, f"{shape} S {s} map {name}: {len(bad)} coordinates differ, first box {boxes[bad[0][0]]}: {gb[bad[0][0]]} vs {wb[bad[0][0]]}"
    finally:
        eng.map_clear()


# ---------------------------------------------------------------------------- 3. n_maps = 0 is lp_run_views
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_mapped_without_maps_equals_run_views(models, prec):
    frames = models["frames"]
    B = len(frames)
    e = _engine(models, prec, B * len(E2E_VIEWS))
    try:
        ref = e.run_views(frames, E2E_VIEWS, CONF, IOU, MIN_AREA)
        ref = (ref[0].copy(), ref[1].copy(), ref[2].copy())
        ref_avg = e.last_det_conf_avg.copy()
        assert int(ref[1].sum()) >= 4, "run_views found too little: the comparison is empty"
        e.map_add(M.rotated(S, H, W, 7.0, 1.3), H, W)   # registered, not listed
        for call in range(3):   # eager, captured, replayed
            got = e.run_mapped(frames, E2E_VIEWS, [], CONF, IOU, MIN_AREA)
            _same_host(got, ref, e.last_det_conf_avg, ref_avg, B, f"{prec} call {call}")
        st = e.graph_stats()
        assert st["replays"] >= 1, st
    finally:
        e.close()


# ---------------------------------------------------------------------------- 4. crop maps against window views
def _crop_frame():
    from litepi import synth
    return np.ascontiguousarray(synth.config4_images(2, seed=CROP_SEED, size=960, grain=8)[CROP_FRAME][:H, :W])


def test_crop_maps_equal_window_views(models):
    """Integer crop maps of the tile grid against lp_run_views on the windows {x0, y0, S, S}: the same pixels reach the detector,
    so counts, det_class and the bits of det_conf are equal; boxes within 1e-3 px (both paths round a coordinate below 4096 at
    most twice, and one ulp there is 4.9e-4); cls_class equal on every record all of whose coordinates, in both results, lie
    at least 2e-3 from an integer (there the ROI's integer rectangle cannot differ), at least three quarters of all records
    (the CPU oracle's share for this frame: CROP_SHARE)."""
    grid = T.tile_grid(S, H, W, 64, False)
    assert len(grid) == 12 and all(w == S and h == S for _, _, w, h in grid)
    assert CROP_SHARE >= 0.75
    frame = _crop_frame()
    e = _engine(models, "fp32", len(grid))
    try:
        ids = [e.map_add(M.crop(S, x, y), H, W) for x, y, _, _ in grid]
        ref = e.run_views([frame], grid, CROP_CONF, IOU, MIN_AREA)
        ref = (ref[0].copy(), ref[1].copy(), ref[2].copy())
        got = e.run_mapped([frame], [], ids, CROP_CONF, IOU, MIN_AREA)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), f"counts {got[1]} / {got[2]} vs {ref[1]} / {ref[2]}"
        n = int(ref[1][0])
        assert n >= 4, "too few detections for a meaningful comparison"
        g, r = got[0][0, :n], ref[0][0, :n]
        assert np.array_equal(g["det_class"], r["det_class"])
        assert np.array_equal(g["det_conf"].view(np.uint32), r["det_conf"].view(np.uint32))
        gb = np.stack([g[k] for k in ("x1", "y1", "x2", "y2")], 1).astype(np.float64)
        rb = np.stack([r[k] for k in ("x1", "y1", "x2", "y2")], 1).astype(np.float64)
        print(f"{n} records, largest box difference {np.abs(gb - rb).max():.3g} px")
        assert np.abs(gb - rb).max() <= 1e-3

        def far(b):
            return np.all(np.abs(b - np.round(b)) >= 2e-3, axis=1)
        sure = far(gb) & far(rb)
        print(f"{int(sure.sum())} of {n} records lie clear of the integers (oracle share {CROP_SHARE})")
        assert sure.sum() >= 0.75 * n
        assert np.array_equal(g["cls_class"][sure], r["cls_class"][sure]) and (g["cls_class"][sure] >= 0).all()
    finally:
        e.close()


# ---------------------------------------------------------------------------- 5. fp32 end to end against the oracle
def test_mapped_fp32_end_to_end_vs_oracle(models):
    """Tolerances of test_views_fp32_end_to_end_vs_oracle: score 1e-3, box 1 px, classes and num_det equal."""
    from litepi import HybridPipeline
    from oracle import ncnn_ref, shufflenet_ref
    frame = models["frames"][E2E_FRAME]
    cpu = M.CpuMappedPipeline(ncnn_ref.load_model(models["param"], models["bin"]), shufflenet_ref.build(91, models["sd"]), input_size=S)
    exp, exp_num = cpu.run_mapped(frame, ["full"], E2E_MAPS(), CONF, IOU, MIN_AREA)
    print(f"oracle: {exp_num} kept after the frame NMS, {len(exp)} after the area filter")
    assert exp_num == E2E_ORACLE_KEPT, f"the oracle keeps {exp_num}, the literal says {E2E_ORACLE_KEPT}"
    assert E2E_ORACLE_KEPT >= 4, "calibration produced too few detections for a meaningful test"
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, det_input_size=S,
                          precision="fp32", max_batch=4, max_det=300, views=["full"], view_maps=E2E_MAPS(), view_maps_frame=(H, W))
    try:
        res, met = pipe.run_batch([frame], CONF, IOU, MIN_AREA)[0]
    finally:
        pipe.engine.close()
    print(f"device: num_det {met.num_detections}, {len(res)} results")
    assert met.num_detections == exp_num, f"num_det {met.num_detections} vs oracle {exp_num}"
    assert len(res) == len(exp), f"{len(res)} results vs oracle {len(exp)}"
    for r, x in zip(res, exp):
        assert abs(r["det_conf"] - x["det_conf"]) <= 1e-3
        assert np.abs(np.array(r["bbox"]) - np.array(x["bbox"])).max() <= 1
        assert r["det_class"] == x["det_class"] and r["cls_class"] == x["cls_class"]


# ---------------------------------------------------------------------------- 6. device path
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_mapped_device_path_equals_host_path(models, fmt):
    import pixfmt_ref as R
    from litepi._ffi import DET_DTYPE
    frames = [models["frames"][0], models["frames"][1]]
    if fmt == "nv12":
        frames = [R.bgr_to_nv12(f) for f in frames]
    B = 2
    e = _engine(models, "fp16", 16)
    try:
        e.set_input_format(fmt)
        ids = [e.map_add(m, H, W) for m in E2E_MAPS() + [M.crop(S, 256, 128), M.rotated(S, H, W, -20.0, 2.0)]]
        lists = {"A": (["full"], ids[:2]), "B": ([], [ids[3], ids[1], ids[2]])}
        refs = {}
        for name, (views, maps) in lists.items():
            d, c, nd, _ = e.run_mapped(frames, views, maps, CONF, IOU, MIN_AREA)
            refs[name] = (d.copy(), c.copy(), nd.copy(), e.last_det_conf_avg.copy())
        assert all(int(r[2].sum()) >= 2 for r in refs.values()), [r[2] for r in refs.values()]
        assert refs["A"][0].tobytes() != refs["B"][0].tobytes()
        buf = torch.from_numpy(np.stack(frames)).cuda()
        dd = torch.zeros(B * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        st0 = e.graph_stats()
        for call, name in enumerate("AAABBB"):   # eager, captured, replayed; another map list: captured anew
            views, maps = lists[name]
            e.run_mapped_device(buf.data_ptr(), B, H, W, views, maps, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            dets_ref, counts_ref, num_ref, avg_ref = refs[name]
            cnt = dc.cpu().numpy()
            tag = f"{fmt} call {call} list {name}"
            assert np.array_equal(cnt[:B], counts_ref) and np.array_equal(cnt[B:2 * B], num_ref), tag
            assert np.array_equal(cnt[2 * B:].view(np.uint32), avg_ref.view(np.uint32)), tag
            recs = dd.cpu().numpy().view(DET_DTYPE).reshape(B, -1)
            for i in range(B):
                assert recs[i, :counts_ref[i]].tobytes() == dets_ref[i, :counts_ref[i]].tobytes(), f"{tag} frame {i}"
            st = e.graph_stats()
            done = {k: st[k] - st0[k] for k in ("eager", "captures", "replays")}
            want = [(1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)][call]
            assert (done["eager"], done["captures"], done["replays"]) == want, f"{tag}: {done}"
    finally:
        e.close()


# ---------------------------------------------------------------------------- 7. pipeline
def test_mapped_pipeline_equals_engine_tracks_and_collects_signs(models):
    from litepi import HybridPipeline
    from oracle import postprocess_ref as P
    rng = np.random.default_rng(3)
    patch = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    seq = []
    for k in range(6):
        f = models["frames"][0].copy()
        f[300:396, 400 + 4 * k:496 + 4 * k] = patch
        seq.append(f)
    maps = E2E_MAPS()
    tcfg = dict(n_streams=1, max_tracks=256, max_age=1, min_hits=2, iou_match=0.3)
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, det_input_size=S,
                          precision="fp16", max_batch=4, max_det=300, views=["full"], view_maps=maps, view_maps_frame=(H, W),
                          track=True, track_config=tcfg, inventory=True, evidence=64)
    e = _engine(models, "fp16", 4, classifier=False)
    try:
        e.load_classifier(models["sd"])
        ids = [e.map_add(m, H, W) for m in maps]
        # two frames of three views on a handle of four: two engine calls; every frame equals Engine.run_mapped on it alone
        outs = pipe.run_batch(seq[:2], CONF, IOU, MIN_AREA, track=False)
        for k in range(2):
            d, c, nd, _ = e.run_mapped([seq[k]], ["full"], ids, CONF, IOU, MIN_AREA)
            res, met = outs[k]
            n = int(c[0])
            assert met.num_detections == int(nd[0]) and len(res) == n and n >= 2, f"frame {k}"
            assert [(r["det_conf"], r["cls_class"], r["cls_conf"]) for r in res] == \
                   [(float(x["det_conf"]), int(x["cls_class"]), float(x["cls_conf"])) for x in d[0, :n]], f"frame {k}"
            assert [r["bbox"] for r in res] == [tuple(int(v) for v in (x["x1"], x["y1"], x["x2"], x["y2"])) for x in d[0, :n]]
        sightings = {}   # (frame number, track id) -> the sighting's classifier crop and its record
        for k, f in enumerate(seq):
            res, _ = pipe.run_batch([f], CONF, IOU, MIN_AREA)[0]
            crops, img, slot = pipe.engine.debug_rois()
            d, c, _, _ = e.run_mapped([f], ["full"], ids, CONF, IOU, MIN_AREA)
            assert len(res) == int(c[0]) and [r["det_conf"] for r in res] == [float(x) for x in d[0, :len(res)]["det_conf"]]
            for r_i, s_i in enumerate(slot.tolist()):
                assert img[r_i] == 0
                sightings[k, res[s_i]["track_id"]] = (crops[r_i].copy(), d[0, s_i].copy())
        signs = pipe.drain_signs(flush=True)
        with_crop = [s for s in signs if s["crop"] is not None]
        assert with_crop, "no sign with a crop came out"
        assert all("evidence" in s and "evidence_window" in s for s in signs)
        n_native = 0
        for s in with_crop:
            crop, rec = sightings[s["best_frame"], s["track_id"]]
            assert s["crop"].tobytes() == crop.tobytes(), f"track {s['track_id']}: the drained crop is not its best sighting's"
            # ... and that crop is cut from the native frame, at the record's frame-coordinate box
            box = np.float32([[rec["x1"], rec["y1"], rec["x2"], rec["y2"]]])
            rects, valid = P.roi_rects(box, H, W, MIN_AREA)
            assert len(rects) == 1
            want = pipe.engine.test_roi_resize_rects(seq[s["best_frame"]], np.asarray(rects, dtype=np.int32))[0]
            assert crop.tobytes() == want.tobytes(), f"track {s['track_id']}: the crop is not cut from the native frame"
            n_native += 1
            if s["evidence"] is not None:
                x, y, w, h = s["evidence_window"]
                assert s["evidence"].shape == (64, 64, 3) and 0 <= x and x + w <= W and 0 <= y and y + h <= H
        assert n_native >= 1 and any(s["evidence"] is not None for s in signs)
    finally:
        pipe.close()
        e.close()


# ---------------------------------------------------------------------------- 8. errors
def test_mapped_errors_leave_the_handle_usable(models):
    from litepi import Engine
    from litepi._ffi import LP_ERR_ARG, LP_ERR_STATE, LitepiError
    frames = models["frames"]
    e = _engine(models, "fp16", 6)
    try:
        ids = [e.map_add(m, H, W) for m in E2E_MAPS()]
        small = e.map_add(M.crop(S, 0, 0), 600, W)   # a map of another frame size
        good = (["full"], ids)
        ref = e.run_mapped(frames, *good, CONF, IOU, MIN_AREA)
        ref = (ref[0].copy(), ref[1].copy(), ref[2].copy())
        ref_avg = e.last_det_conf_avg.copy()
        dd = torch.zeros(2 * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(6, dtype=torch.int32, device="cuda")
        dev = torch.from_numpy(np.stack(frames)).cuda()
        torch.cuda.synchronize()
        bad_calls = {"a map of another frame size": (["full"], [ids[0], small]),
                     "an unknown id": (["full"], [ids[0], 3]),
                     "a negative id": ([], [-1]),
                     "no view and no map": ([], []),
                     "B x (n_views + n_maps) > max_batch": (["full", (0, 0, 320, 320)], ids),
                     "a bad window in front of good maps": ([(600, 40, 297, 100)], ids)}
        for what, bad in bad_calls.items():
            with pytest.raises(LitepiError) as ex:
                e.run_mapped(frames, *bad, CONF, IOU, MIN_AREA)
            assert ex.value.code == LP_ERR_ARG, what
            got = e.run_mapped(frames, *good, CONF, IOU, MIN_AREA)   # the handle is still usable, with the same result
            _same_host(got, ref, e.last_det_conf_avg, ref_avg, 2, f"after {what}")
            with pytest.raises(LitepiError) as ex:
                e.run_mapped_device(dev.data_ptr(), 2, H, W, *bad, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
            assert ex.value.code == LP_ERR_ARG, what + " (device)"
            e.run_mapped_device(dev.data_ptr(), 2, H, W, *good, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            assert np.array_equal(dc.cpu().numpy()[:2], ref[1]), f"device call after {what}"
        # every frame of the call counts: the second frame is smaller than the maps' frame size
        with pytest.raises(LitepiError) as ex:
            e.run_mapped([frames[0], np.ascontiguousarray(frames[1][:600])], *good, CONF, IOU, MIN_AREA)
        assert ex.value.code == LP_ERR_ARG
        # ... and the smaller frame alone goes with its own map
        e.run_mapped([np.ascontiguousarray(frames[1][:600])], [], [small], CONF, IOU, MIN_AREA)
        # a NaN in a table; ids dropped by map_clear
        nan = M.crop(S, 0, 0)
        nan[7, 9, 1] = np.nan
        with pytest.raises(LitepiError) as ex:
            e.map_add(nan, H, W)
        assert ex.value.code == LP_ERR_ARG
        with pytest.raises(LitepiError) as ex:
            e.test_map_boxes(17, np.zeros((1, 4), np.float32))
        assert ex.value.code == LP_ERR_ARG
        e.map_clear()
        with pytest.raises(LitepiError) as ex:
            e.run_mapped(frames, ["full"], [0], CONF, IOU, MIN_AREA)
        assert ex.value.code == LP_ERR_ARG
        assert e.map_add(E2E_MAPS()[0], H, W) == 0 and e.map_add(E2E_MAPS()[1], H, W) == 1   # ids start again
        got = e.run_mapped(frames, *good, CONF, IOU, MIN_AREA)
        _same_host(got, ref, e.last_det_conf_avg, ref_avg, 2, "after map_clear")
        for k in range(2, 64):
            assert e.map_add(np.zeros((S, S, 2), np.float32), H, W) == k
        with pytest.raises(LitepiError) as ex:   # LP_MAP_MAX
            e.map_add(np.zeros((S, S, 2), np.float32), H, W)
        assert ex.value.code == LP_ERR_STATE
        got = e.run_mapped(frames, *good, CONF, IOU, MIN_AREA)
        _same_host(got, ref, e.last_det_conf_avg, ref_avg, 2, "with LP_MAP_MAX maps")
    finally:
        e.close()
    r = Engine(precision="fp16", max_batch=2, max_det=8, num_classes=4, det_input=(192, 320))   # a rectangular handle
    try:
        for call in (lambda: r.map_add(M.crop(320, 0, 0), H, W), lambda: r.run_mapped(frames, ["full"], [], CONF, IOU, MIN_AREA),
                     lambda: r.run_mapped_device(0, 1, H, W, ["full"], [], CONF, IOU, MIN_AREA, 0, 0),
                     lambda: r.test_map_views(frames[0], [0]), lambda: r.test_map_boxes(0, np.zeros((1, 4), np.float32))):
            with pytest.raises(LitepiError) as ex:
                call()
            assert ex.value.code == LP_ERR_STATE
    finally:
        r.close()


def test_mapped_list_beyond_the_frame_nms_capacity(models):
    """2100 anchors at det_input 320: the frame NMS's flag masks hold 292 views of one frame; 293 are LP_ERR_ARG before anything
    is enqueued, on a handle whose max_batch would hold them"""
    from litepi import Engine
    from litepi._ffi import LP_ERR_ARG, LitepiError
    e = Engine(precision="fp16", max_batch=296, max_det=300, num_classes=91, det_input=S, max_rois=300)
    try:
        e.load_detector(models["param"], models["bin"])
        a = e.map_add(M.crop(S, 100, 100), H, W)
        b = e.map_add(M.crop(S, 300, 200), H, W)
        dev = torch.from_numpy(models["frames"][0]).cuda()
        dd = torch.zeros(e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(LitepiError) as ex:
            e.run_mapped_device(dev.data_ptr(), 1, H, W, [], [a, b] * 146 + [a], CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
        assert ex.value.code == LP_ERR_ARG and "capacity" in str(ex.value)
        e.run_mapped_device(dev.data_ptr(), 1, H, W, [], [a, b], CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
        e.synchronize()
        assert int(dc.cpu().numpy()[1]) >= 1
    finally:
        e.close()


# ---------------------------------------------------------------------------- 9. nothing changes when unused
def test_maps_change_nothing_where_they_are_not_listed(models):
    """the lp_det bytes and the profiled launch list of lp_run_batch and lp_run_views are equal before lp_map_add, with maps
    registered and after lp_map_clear"""
    frames = models["frames"]
    e = _engine(models, "fp16", 8)
    try:
        def state():
            out = {}
            for name, call in (("run_batch", lambda: e.run_batch(frames, CONF, IOU, MIN_AREA)),
                               ("run_views", lambda: e.run_views(frames, E2E_VIEWS, CONF, IOU, MIN_AREA))):
                d, c, nd, _ = call()
                e.profile_next(True)
                d2, c2, _, _ = call()
                launches = [(r["name"], r["layer"]) for r in e.profile_read()]
                used = lambda dets, cnt: b"".join(dets[i, :int(cnt[i])].tobytes() for i in range(len(frames)))   # noqa: E731
                assert used(d, c) == used(d2, c2) and c.tolist() == c2.tolist() and launches
                out[name] = (used(d, c), c.tolist(), nd.tolist(), launches)
            return out
        before = state()
        assert sum(before["run_views"][1]) >= 4
        assert not any("map" in n for n, _ in before["run_views"][3])
        ids = [e.map_add(m, H, W) for m in E2E_MAPS()]
        with_maps = state()
        e.profile_next(True)
        e.run_mapped(frames, ["full"], ids, CONF, IOU, MIN_AREA)   # ... and a call that lists them books the two new launches
        names = [(r["name"], r["layer"]) for r in e.profile_read()]
        assert ("map_views_u8", "view_gather") in names and ("map_candidates", "nms") in names
        foot = 0   # booked: table + view + the bounding rectangle of every table's taps inside the frame
        for m in E2E_MAPS():
            fx = M.fixed(m, H, W)
            ix0, ix1 = np.clip(fx[..., 0] >> 5, 0, None), np.clip((fx[..., 0] >> 5) + 1, None, W - 1)
            iy0, iy1 = np.clip(fx[..., 1] >> 5, 0, None), np.clip((fx[..., 1] >> 5) + 1, None, H - 1)
            foot += 3 * int(ix1.max() - ix0.min() + 1) * int(iy1.max() - iy0.min() + 1)
        assert [r for r in e.profile_read() if r["name"] == "map_views_u8"][0]["bytes"] == 2 * (2 * S * S * 11 + foot)
        used = state()
        e.map_clear()
        after = state()
        for tag, st in (("with maps registered", with_maps), ("after a mapped call", used), ("after lp_map_clear", after)):
            for name in before:
                assert st[name][:3] == before[name][:3], f"{name} {tag}: records differ"
                assert st[name][3] == before[name][3], f"{name} {tag}: launch list differs"
    finally:
        e.close()
