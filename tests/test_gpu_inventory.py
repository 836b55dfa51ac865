"""GPU tests of the sign inventory (include/litepi.h, lp_inventory_*): the device inventory against the NumPy restatement of
the rule (tests/inventory_ref.py).  Both sides do the same fp32 operations on the same records, so every comparison is exact:
integers equal, floats bit-equal, crops byte-equal.

1. rule: lp_track then lp_inventory(crops = 0) on synthetic record streams == the reference, log and open entries;
2. crops, model-free: ROI lists installed with lp_test_set_rois (records omitted, images shuffled, stale entries beyond total);
3. streams do not interact; 64 streams x 1 frame; 12 device calls enqueued without a synchronise == the same fed one by one;
4. a full log: order, `dropped`, a drain re-arms it;
5. lp_run_batch_device / lp_run_tiled_device / NV12 -> lp_track_device -> lp_inventory_device(crops = 1) == the reference fed the
   downloaded records and lp_debug_rois crops;
6. an inventory changes no tracker output and no launch list; 7. argument errors; 8. HybridPipeline and e2e --inventory."""
import csv
import itertools
import json

import numpy as np
import pytest
import torch

import inventory_ref as V
import pixfmt_ref as P
import tracking_ref as R

pytestmark = pytest.mark.gpu

NC = 58
S = 64


# ---------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def engines():
    """handles without models (the inventory needs none), keyed by max_det"""
    from litepi import Engine
    es = {md: Engine(precision="fp16", max_batch=64, max_det=md, num_classes=NC) for md in (16, 300)}
    yield es
    for e in es.values():
        e.close()


def assert_signs_equal(got, want, tag):
    assert len(got) == len(want), f"{tag}: {len(got)} signs, want {len(want)}"
    for name in got.dtype.names:
        bad = np.flatnonzero(got[name].view(np.int32) != want[name].view(np.int32))
        assert len(bad) == 0, f"{tag}: field {name}, sign {bad[0]}: got {got[name][bad[0]]!r}, want {want[name][bad[0]]!r}"


def assert_drain_equal(eng, ref, tag, by_stream=False, crops=True):
    gs, gc, gd = eng.inventory_drain(crops=crops)
    ws, wc, wd = ref.drain()
    if by_stream:   # across the streams of a call the order of blocks is unspecified
        go, wo = np.argsort(gs["stream"], kind="stable"), np.argsort(ws["stream"], kind="stable")
        gs, ws, wc = gs[go], ws[wo], wc[wo]
        gc = gc[go] if gc is not None else None
    assert_signs_equal(gs, ws, tag)
    assert gd == wd, f"{tag}: dropped {gd}, want {wd}"
    if crops:
        assert gc.shape == wc.shape and gc.tobytes() == wc.tobytes(), f"{tag}: crops differ"
    return gs


def create(eng, tcfg, icfg):
    eng.tracker_create(**tcfg)
    eng.inventory_create(**icfg)


# ---------------------------------------------------------------------------- 1. the rule
RULE_CONFIGS = [dict(max_age=a, min_hits=h, max_tracks=t, best=b, max_det=md)
                for a, h, t, b, md in itertools.product((0, 3), (1, 3), (4, 256), (0, 1, 2), (16, 300))]


def rule_id(k):
    c = RULE_CONFIGS[k]
    return f"{k}-a{c['max_age']}h{c['min_hits']}t{c['max_tracks']}b{c['best']}md{c['max_det']}"


@pytest.mark.parametrize("k", range(len(RULE_CONFIGS)), ids=rule_id)
def test_rule_equals_reference(engines, k):
    c = RULE_CONFIGS[k]
    md, eng = c["max_det"], engines[c["max_det"]]
    dets, counts = R.make_scene(1000 * k + 7, max_det=md, num_classes=NC)
    assert 40 <= len(counts) <= 200
    # the inventory's own min_hits on the AREA cases, the tracker's (min_hits = 0) on the others
    own = c["best"] == V.BEST_AREA
    tcfg = dict(max_tracks=c["max_tracks"], max_age=c["max_age"], min_hits=2 if own else c["min_hits"])
    icfg = dict(best=c["best"], min_hits=c["min_hits"] if own else 0, keep_crops=0)
    create(eng, tcfg, icfg)
    ref = V.InventoryRef(md, tcfg, icfg)
    logged = 0
    for i in range(0, len(counts), 32):
        d, n = dets[i:i + 32], counts[i:i + 32]
        tracks = eng.track(d, n)
        eng.inventory(d, n, tracks)
        ref.feed(d, tracks, n)
        logged += len(assert_drain_equal(eng, ref, f"{rule_id(k)} call {i // 32}", crops=False))
        op = eng.inventory_open(0)
        assert_signs_equal(op, ref.open(0), f"{rule_id(k)} open entries after call {i // 32}")
        snap = eng.tracker_snapshot(0)["tracks"]
        assert [s for s, _, _ in ref.open_state(0)] == snap["slot"].tolist()
        assert (op["track_id"].tolist(), op["hits"].tolist()) == (snap["track_id"].tolist(), snap["hits"].tolist())
    eng.inventory_flush()
    ref.flush()
    rest = assert_drain_equal(eng, ref, f"{rule_id(k)} flush", crops=False)
    assert len(eng.inventory_open(0)) == 0 and (rest["flags"] & V.FLUSHED).all()
    assert logged + len(rest) > 0


# ---------------------------------------------------------------------------- 2. crops, model-free
def make_rois(rng, call, counts, max_det, omit=0.3):
    """a ROI list over the call's records in shuffled image order with a share of the records omitted, and crops whose bytes
    encode (call, frame, record); returns the kept list and the omitted entries"""
    recs = [(b, i) for b in rng.permutation(len(counts)) for i in range(counts[b])]
    keep = rng.random(len(recs)) >= omit
    kept = [r for r, k in zip(recs, keep) if k]
    left = [r for r, k in zip(recs, keep) if not k]

    def crops_of(rs):
        c = rng.integers(0, 256, (len(rs), S, S, 3), dtype=np.uint8)
        for j, (b, i) in enumerate(rs):
            c[j, 0, 0] = (call, b, i % 256)
        return c
    return kept, crops_of(kept), left, crops_of(left)


@pytest.mark.parametrize("md, best", [(16, V.BEST_AREA), (300, V.BEST_CLS_CONF), (16, V.BEST_DET_CONF)])
def test_crops_model_free(engines, md, best):
    eng = engines[md]
    rng = np.random.default_rng(5 + md)
    dets, counts = R.make_scene(3100 + md, max_det=md, num_classes=NC, n_frames=64, n_signs=14)
    tcfg, icfg = dict(max_tracks=16, max_age=1, min_hits=1), dict(best=best)
    create(eng, tcfg, icfg)
    ref = V.InventoryRef(md, tcfg, icfg)
    with_crop = without = 0
    for call, i in enumerate(range(0, 64, 16)):
        d, n = dets[i:i + 16], counts[i:i + 16]
        kept, kc, left, lc = make_rois(rng, call, n, md)
        # the whole list first, then its kept part alone: the omitted records stay behind `total` as stale entries
        both = kept + left
        eng.test_set_rois(np.concatenate([kc, lc]), [b for b, _ in both], [s for _, s in both])
        eng.test_set_rois(kc, [b for b, _ in kept], [s for _, s in kept])
        got = eng.debug_rois()
        assert got[0].tobytes() == kc.tobytes() and got[1].tolist() == [b for b, _ in kept] and got[2].tolist() == [s for _, s in kept]
        tracks = eng.track(d, n)
        eng.inventory(d, n, tracks, crops=True)
        ref.feed(d, tracks, n, crops=V.rois_to_crops(kc, [b for b, _ in kept], [s for _, s in kept]))
        signs = assert_drain_equal(eng, ref, f"call {call}")
        with_crop += int((signs["flags"] & V.HAS_CROP).sum())
        without += int(((signs["flags"] & V.HAS_CROP) == 0).sum())
        assert_signs_equal(eng.inventory_open(0), ref.open(0), f"open entries after call {call}")
    eng.inventory_flush()
    ref.flush()
    signs = assert_drain_equal(eng, ref, "flush")
    with_crop += int((signs["flags"] & V.HAS_CROP).sum())
    without += int(((signs["flags"] & V.HAS_CROP) == 0).sum())
    assert with_crop > 0 and without > 0, "the scene must log signs of both kinds"


# ---------------------------------------------------------------------------- 3. streams and depth
def test_interleaved_streams_equal_each_stream_alone(engines):
    tcfg, icfg = dict(max_tracks=16, max_age=2, min_hits=1), dict(keep_crops=0, best=V.BEST_DET_CONF)
    eng = engines[16]
    scenes = [R.make_scene(s, max_det=16, num_classes=NC, n_frames=21, n_signs=6) for s in (501, 502, 503)]
    sids = [4, 0, 2]
    order = np.random.default_rng(8).permutation(np.repeat(np.arange(3), 21))
    pos = [0, 0, 0]
    dets, counts = np.zeros((63, 16), dtype=R.DET_DTYPE), np.zeros(63, np.int32)
    for b, q in enumerate(order):
        dets[b], counts[b] = scenes[q][0][pos[q]], scenes[q][1][pos[q]]
        pos[q] += 1
    stream_ids = np.array([sids[q] for q in order], np.int32)
    create(eng, dict(tcfg, n_streams=5), icfg)
    ref = V.InventoryRef(16, dict(tcfg, n_streams=5), icfg)
    tracks = eng.track(dets, counts, stream_ids)
    eng.inventory(dets, counts, tracks, stream_ids)
    eng.inventory_flush()
    ref.feed(dets, tracks, counts, stream_ids)
    ref.flush()
    both = assert_drain_equal(eng, ref, "interleaved", by_stream=True, crops=False)
    assert len(both) > 6
    for q in range(3):
        create(eng, tcfg, icfg)
        eng.inventory(*scenes[q], eng.track(*scenes[q]))
        eng.inventory_flush()
        alone = eng.inventory_drain(crops=False)[0]
        alone["stream"] = sids[q]
        assert_signs_equal(both[both["stream"] == sids[q]], alone, f"sequence {q} alone")


def test_64_streams_one_frame_per_call(engines):
    tcfg, icfg = dict(max_tracks=8, max_age=1, n_streams=64, min_hits=2), dict(keep_crops=0)
    eng = engines[16]
    scenes = [R.make_scene(9000 + s, max_det=16, num_classes=NC, n_frames=40, n_signs=5) for s in range(64)]
    create(eng, tcfg, icfg)
    ref = V.InventoryRef(16, tcfg, icfg)
    sid = np.arange(64, dtype=np.int32)[::-1].copy()
    total = 0
    for t in range(40):
        dets = np.stack([scenes[s][0][t] for s in sid])
        counts = np.array([scenes[s][1][t] for s in sid], np.int32)
        tracks = eng.track(dets, counts, sid)
        eng.inventory(dets, counts, tracks, sid)
        ref.feed(dets, tracks, counts, sid)
        if t % 8 == 7:
            total += len(assert_drain_equal(eng, ref, f"call {t}", by_stream=True, crops=False))
    for s in (0, 17, 63):
        assert_signs_equal(eng.inventory_open(s), ref.open(s), f"open entries of stream {s}")
    eng.inventory_flush(17)
    ref.flush(17)
    assert len(eng.inventory_open(17)) == 0 and len(eng.inventory_open(16)) == len(ref.open(16))
    eng.inventory_flush()
    ref.flush()
    total += len(assert_drain_equal(eng, ref, "flush", by_stream=True, crops=False))
    assert total > 64


def test_12_device_calls_in_flight_equal_one_by_one(engines):
    from litepi._ffi import TRACK_DTYPE
    tcfg, icfg = dict(max_tracks=32, max_age=1, min_hits=1, n_streams=2), dict(best=V.BEST_AREA)
    eng = engines[16]
    dev = torch.device("cuda", 0)
    dets, counts = R.make_scene(4242, max_det=16, num_classes=NC, n_frames=96, n_signs=20)
    sid = np.array([0, 1] * 4, np.int32)
    rng = np.random.default_rng(3)
    create(eng, tcfg, icfg)
    bufs = []
    for k in range(12):
        d, n = dets[8 * k:8 * k + 8], counts[8 * k:8 * k + 8]
        bufs.append((torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).to(dev), torch.from_numpy(n.copy()).to(dev),
                     torch.zeros(8 * 16 * 32, dtype=torch.uint8, device=dev)))
    # one ROI list for all calls (the handle's crop buffer does not change while the calls are in flight)
    kept, kc, _, _ = make_rois(rng, 0, np.full(8, 16), 16, omit=0.2)
    eng.test_set_rois(kc, [b for b, _ in kept], [s for _, s in kept])
    crops = V.rois_to_crops(kc, [b for b, _ in kept], [s for _, s in kept])
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.set_stream(st.cuda_stream)
    try:
        with torch.cuda.stream(st):
            for d, n, t in bufs:   # 12 calls, more than the ring of 8, without a synchronise
                eng.track_device(d.data_ptr(), n.data_ptr(), 8, t.data_ptr(), sid)
                eng.inventory_device(d.data_ptr(), n.data_ptr(), t.data_ptr(), 8, sid, crops=True)
            eng.inventory_flush()
        eng.synchronize()
        torch.cuda.synchronize()
        deep = eng.inventory_drain()
        tracks = [t.cpu().numpy().view(TRACK_DTYPE).reshape(8, 16) for _, _, t in bufs]
    finally:
        eng.set_stream(0)
    create(eng, tcfg, icfg)
    ref = V.InventoryRef(16, tcfg, icfg)
    for k in range(12):
        d, n = dets[8 * k:8 * k + 8], counts[8 * k:8 * k + 8]
        eng.inventory(d, n, tracks[k], sid, crops=True)
        eng.synchronize()
        ref.feed(d, tracks[k], n, sid, crops=crops)
    eng.inventory_flush()
    ref.flush()
    one = eng.inventory_drain()
    a, b = np.argsort(deep[0]["stream"], kind="stable"), np.argsort(one[0]["stream"], kind="stable")
    assert_signs_equal(deep[0][a], one[0][b], "12 calls deep vs one by one")
    assert deep[1][a].tobytes() == one[1][b].tobytes() and deep[2] == one[2] == 0
    ws, wc, _ = ref.drain()
    c = np.argsort(ws["stream"], kind="stable")
    assert_signs_equal(one[0][b], ws[c], "one by one vs reference")
    assert one[1][b].tobytes() == wc[c].tobytes() and len(ws) > 12 and (ws["flags"] & V.HAS_CROP).any()


# ---------------------------------------------------------------------------- 4. a full log
def test_log_full(engines):
    tcfg, icfg = dict(max_tracks=64, max_age=0, min_hits=1), dict(max_signs=4, best=V.BEST_AREA)
    eng = engines[16]
    rng = np.random.default_rng(11)
    dets, counts = R.make_scene(2000, max_det=16, num_classes=NC, n_frames=96, n_signs=30)
    create(eng, tcfg, icfg)
    ref = V.InventoryRef(16, tcfg, icfg)
    dropped, logged = 0, 0
    for call, i in enumerate(range(0, 96, 8)):
        d, n = dets[i:i + 8], counts[i:i + 8]
        kept, kc, _, _ = make_rois(rng, call, n, 16, omit=0.1)
        eng.test_set_rois(kc, [b for b, _ in kept], [s for _, s in kept])
        tracks = eng.track(d, n)
        eng.inventory(d, n, tracks, crops=True)
        ref.feed(d, tracks, n, crops=V.rois_to_crops(kc, [b for b, _ in kept], [s for _, s in kept]))
        if call % 3 == 2:   # the log overflows between two drains and is armed again by each
            want_drop = ref.dropped
            signs = assert_drain_equal(eng, ref, f"drain after call {call}")
            assert len(signs) <= 4
            dropped += want_drop
            logged += len(signs)
    assert dropped > 0 and logged >= 8, "the scene must overflow a log of 4 signs"
    nlog = eng.inventory_drain(crops=False)
    assert len(nlog[0]) == 0 and nlog[2] == 0, "a drain leaves the log empty"


# ---------------------------------------------------------------------------- models of the pipeline tests
CONF, IOU, MIN_AREA = 0.25, 0.45, 50
N_CALLS, N_FRAMES = 6, 4


def moving_patch(base, rng, step=4):
    """N_CALLS versions of the frames `base` with a pasted patch that moves `step` pixels to the right per call"""
    patch = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    out = []
    for k in range(N_CALLS):
        f = base.copy()
        f[:, 200:296, 160 + step * k:256 + step * k] = patch
        out.append(f)
    return out


@pytest.fixture(scope="module")
def clips():
    rng = np.random.default_rng(77)
    plain = moving_patch(rng.integers(0, 256, (N_FRAMES, 640, 640, 3), dtype=np.uint8), rng)
    nv_bgr = moving_patch(rng.integers(0, 256, (N_FRAMES, 640, 640, 3), dtype=np.uint8), rng)
    nv = [np.stack([P.bgr_to_nv12(f) for f in call]) for call in nv_bgr]
    big = moving_patch(rng.integers(0, 256, (N_FRAMES, 800, 1000, 3), dtype=np.uint8), rng)
    return {"plain": plain, "nv12": nv, "nv12_bgr": [np.stack([P.nv12_to_bgr(f, "bt601") for f in call]) for call in nv], "tiled": big}


@pytest.fixture(scope="module")
def models(tmp_path_factory, clips):
    """a seeded v1 detector whose class bias is shifted so that on the first and the last call's frames of every clip at least
    three anchors pass conf 0.25 with a margin of 0.1 in the logit, measured with the device's own scores (as
    tests/test_gpu_tracking.py), and a seeded classifier"""
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    d = tmp_path_factory.mktemp("inventory_models")
    sd = random_shufflenet_state(91, seed=3)
    cls_file = str(d / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, cls_file)
    every = [f for name in ("plain", "nv12_bgr", "tiled") for k in (0, N_CALLS - 1) for f in clips[name][k]]
    p, b = str(d / "v1.param"), str(d / "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=4321, cls_bias=0.0)
    e = Engine(precision="fp16", max_batch=len(every), max_det=300, num_classes=91)
    try:
        e.load_detector(p, b)
        lb = np.stack([e.test_letterbox(f)[0] for f in every])
        s = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64), axis=1)[:, ::-1]
    finally:
        e.close()
    third = s[:, 2].min()
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - (np.log(third / (1 - third)) - 0.1)))
    return {"cls": sd, "cls_file": cls_file, "v1": (p, b)}


def _engine(models, max_batch=16):
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=max_batch, max_det=300, num_classes=91)
    e.load_detector(*models["v1"])
    e.load_classifier(models["cls"])
    return e


# ---------------------------------------------------------------------------- 5. behind the pipeline
@pytest.mark.parametrize("mode", ["plain", "tiled", "nv12"])
def test_inventory_device_behind_the_pipeline(models, clips, mode):
    from litepi._ffi import DET_DTYPE, TRACK_DTYPE
    dev = torch.device("cuda", 0)
    calls = clips[mode]
    B = len(calls[0])
    tcfg, icfg = dict(n_streams=B, max_tracks=256, max_age=0, min_hits=2, iou_match=0.5), dict(best=V.BEST_AREA)
    sid = np.arange(B, dtype=np.int32)
    eng = _engine(models, max_batch=32 if mode == "tiled" else 16)   # tiled: the views of four 800 x 1000 frames
    try:
        if mode == "nv12":
            eng.set_input_format("nv12", "bt601")
        H, W = (800, 1000) if mode == "tiled" else (640, 640)
        create(eng, tcfg, icfg)
        ref = V.InventoryRef(300, tcfg, icfg)
        d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        t = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        for k, frames in enumerate(calls):
            x = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
            if mode == "tiled":
                eng.run_tiled_device(x.data_ptr(), B, H, W, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr(), overlap=128)
            else:
                eng.run_batch_device(x.data_ptr(), B, H, W, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
            eng.track_device(d.data_ptr(), c.data_ptr(), B, t.data_ptr(), sid)
            eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=True)
            crops, img, slot = eng.debug_rois()   # synchronises
            counts = c.cpu().numpy()[:B].copy()
            dets = d.cpu().numpy().view(DET_DTYPE).reshape(B, 300)
            tracks = t.cpu().numpy().view(TRACK_DTYPE).reshape(B, 300)
            assert len(img) == counts.sum(), f"{mode} call {k}: every kept record has a ROI"
            ref.feed(dets, tracks, counts, sid, crops=V.rois_to_crops(crops, img, slot))
        eng.inventory_flush()
        ref.flush()
        signs = assert_drain_equal(eng, ref, mode, by_stream=True)
        assert (signs["flags"] & V.HAS_CROP).sum() >= 1, f"{mode}: no sign with a crop came out"
        assert ((signs["flags"] & V.FLUSHED) != 0).any()
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 6. nothing else moves
def test_inventory_changes_no_tracker_output_and_no_launch_list(models, clips):
    base = clips["plain"][0]
    B = len(base)
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(base).to(dev)
    dets, counts = R.make_scene(77, max_det=300, num_classes=91, n_frames=16, n_signs=6)
    results = []
    for with_inventory in (False, True):
        eng = _engine(models)
        try:
            eng.tracker_create(max_tracks=64, max_age=1)
            if with_inventory:
                eng.inventory_create()
            d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
            c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
            outs = []
            for call in range(3):   # eager, capture, replay
                eng.run_batch_device(x.data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
                eng.synchronize()
                outs.append((d.cpu().numpy().tobytes(), c.cpu().numpy().tobytes()))
            eng.profile_next(True)
            eng.run_batch_device(x.data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
            eng.synchronize()
            launches = [(r["name"], r["layer"]) for r in eng.profile_read()]
            tracks = eng.track(dets, counts)
            if with_inventory:
                eng.inventory(dets, counts, tracks)
            more = eng.track(dets, counts)
            snap = eng.tracker_snapshot(0)
            results.append((outs, launches, tracks.tobytes(), more.tobytes(), snap["tracks"].tobytes(), snap["acc"].tobytes(), snap["next_id"]))
        finally:
            eng.close()
    assert results[0][0] == results[1][0], "lp_run_batch_device output differs on a handle that has an inventory"
    assert results[0][1] == results[1][1] and len(results[0][1]) > 10, "the launch list differs on a handle that has an inventory"
    assert not any("inventory" in name for name, _ in results[1][1])
    assert results[0][2:] == results[1][2:], "the tracker's output differs on a handle that has an inventory"


# ---------------------------------------------------------------------------- 7. errors
def test_errors_leave_the_handle_usable():
    from litepi import Engine, _ffi
    from litepi._ffi import LitepiError
    eng = Engine(precision="fp16", max_batch=4, max_det=16, num_classes=NC)
    try:
        dets, counts = R.make_scene(31, max_det=16, num_classes=NC, n_frames=8, n_signs=3)
        dev = torch.device("cuda", 0)
        d = torch.from_numpy(dets[:4].view(np.uint8).reshape(-1).copy()).to(dev)
        c = torch.from_numpy(counts[:4].copy()).to(dev)
        t = torch.zeros(4 * 16 * 32 + 16, dtype=torch.uint8, device=dev)
        zeros = np.zeros((4, 16), dtype=R.TRACK_DTYPE)

        def code(fn):
            with pytest.raises(LitepiError) as ei:
                fn()
            return ei.value.code

        # no tracker, then no inventory
        assert code(lambda: eng.inventory_create()) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.inventory(dets[:4], counts[:4], zeros)) == _ffi.LP_ERR_STATE
        tcfg = dict(n_streams=2, max_tracks=8, max_age=1, min_hits=1)
        eng.tracker_create(**tcfg)
        assert code(lambda: eng.inventory(dets[:4], counts[:4], zeros)) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), 4)) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.inventory_flush()) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.inventory_drain()) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.inventory_open(0)) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.inventory_create(max_signs=0)) == _ffi.LP_ERR_ARG
        eng.inventory_destroy()   # without one: fine
        icfg = dict(keep_crops=0, max_signs=64)
        eng.inventory_create(**icfg)
        ref = V.InventoryRef(16, tcfg, icfg)
        tracks = eng.track(dets[:4], counts[:4])
        eng.inventory(dets[:4], counts[:4], tracks)
        ref.feed(dets[:4], tracks, counts[:4])
        # refused before anything is enqueued: the state is untouched
        assert code(lambda: eng.inventory(dets[:4], counts[:4], tracks, crops=True)) == _ffi.LP_ERR_ARG   # keep_crops = 0
        assert code(lambda: eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), 4, crops=True)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), 5)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), 0)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr() + 8, 4)) == _ffi.LP_ERR_ARG   # misaligned
        assert code(lambda: eng.inventory_device(d.data_ptr() + 4, c.data_ptr(), t.data_ptr(), 4)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), 4, [0, 1, 2, 0])) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory(dets[:4], counts[:4], tracks, [0, -1, 0, 0])) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory_flush(2)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory_open(2)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.inventory_open(-1)) == _ffi.LP_ERR_ARG
        assert_signs_equal(eng.inventory_open(0), ref.open(0), "after the refused calls")
        tracks = eng.track(dets[4:8], counts[4:8])
        eng.inventory(dets[4:8], counts[4:8], tracks)
        ref.feed(dets[4:8], tracks, counts[4:8])
        eng.inventory_flush()
        ref.flush()
        # a short cap consumes nothing
        import ctypes as C
        n, dropped = C.c_int(), C.c_int()
        out = np.zeros(64, dtype=_ffi.SIGN_DTYPE)
        assert eng.lib.lp_inventory_drain(eng._h, None, None, 0, C.byref(n), C.byref(dropped)) == 0 and n.value > 1
        assert eng.lib.lp_inventory_drain(eng._h, out.ctypes.data, None, n.value - 1, C.byref(n), C.byref(dropped)) == _ffi.LP_ERR_ARG
        assert eng.lib.lp_inventory_drain(eng._h, out.ctypes.data, out.ctypes.data, 64, C.byref(n), None) == _ffi.LP_ERR_ARG   # no crops kept
        assert_drain_equal(eng, ref, "after the refused drains", crops=False)
        # the inventory goes with its tracker
        eng.tracker_create(**tcfg)
        assert not hasattr(eng, "inv_cfg")
        assert code(lambda: eng.inventory_open(0)) == _ffi.LP_ERR_STATE
        eng.inventory_create(**icfg)
        eng.tracker_reset()   # leaves the inventory alone
        assert len(eng.inventory_open(0)) == 0
        eng.tracker_destroy()
        assert code(lambda: eng.inventory_flush()) == _ffi.LP_ERR_STATE
    finally:
        eng.close()


def test_tracker_reset_orphans_close_by_the_rule(engines):
    tcfg, icfg = dict(max_tracks=16, max_age=2, min_hits=1), dict(keep_crops=0)
    eng = engines[16]
    dets, counts = R.make_scene(77, max_det=16, num_classes=NC, n_frames=40, n_signs=6)
    create(eng, tcfg, icfg)
    ref = V.InventoryRef(16, tcfg, icfg)
    for i in (0, 20):
        d, n = dets[i:i + 20], counts[i:i + 20]
        tracks = eng.track(d, n)
        eng.inventory(d, n, tracks)
        ref.feed(d, tracks, n)
        if i == 0:
            assert len(eng.inventory_open(0)) > 0
            eng.tracker_reset()
    eng.inventory_flush()
    ref.flush()
    signs = assert_drain_equal(eng, ref, "across a tracker reset", crops=False)
    assert signs["first_frame"].max() >= 20 and len(set(signs["track_id"].tolist())) == len(signs)


# ---------------------------------------------------------------------------- 8. Python and CLI
SIGN_KEYS = {"stream", "track_id", "first_frame", "last_frame", "hits", "cls", "cls_conf", "bbox", "det_class", "best_frame", "crop", "flushed"}


def test_hybrid_pipeline_drain_signs(models, clips):
    from litepi import HybridPipeline
    p, b = models["v1"]
    kw = dict(num_classes=91, precision="fp16", max_batch=16, max_det=300)
    calls = [list(c) for c in clips["plain"]]
    B = len(calls[0])
    tcfg = dict(n_streams=B, max_tracks=256, max_age=0, min_hits=2, iou_match=0.5)
    sid = list(range(B))
    with pytest.raises(ValueError, match="track"):
        HybridPipeline(p, b, models["cls_file"], "shufflenetv2", inventory=True, **kw)
    pipe = HybridPipeline(p, b, models["cls_file"], "shufflenetv2", track=True, track_config=tcfg, inventory=dict(best="area"), **kw)
    try:
        ref = V.InventoryRef(300, tcfg, dict(best=V.BEST_AREA))
        trk = R.TrackerRef(max_det=300, num_classes=91, **tcfg)
        got = []
        for k, imgs in enumerate(calls):
            pipe.run_batch(imgs, CONF, IOU, MIN_AREA, stream_ids=sid)
            crops, img, slot = pipe.engine.debug_rois()
            pipe.run_batch(imgs, CONF, IOU, MIN_AREA, track=False)   # not tracked: the inventory is not fed
            dets, counts, _, _ = pipe.engine.run_batch(imgs, CONF, IOU, MIN_AREA)
            ref.feed(dets[:B], trk.track(dets[:B], counts[:B].astype(np.int32), sid), counts[:B], sid, crops=V.rois_to_crops(crops, img, slot))
            if k == 3:
                got += pipe.drain_signs()
        got += pipe.drain_signs(flush=True)
        ref.flush()
        ws, wc, _ = ref.drain()
        assert len(got) == len(ws) and len(got) >= 3 and all(set(s) == SIGN_KEYS for s in got)
        key = lambda s: (s["stream"], s["track_id"])
        want = sorted(({"stream": int(s["stream"]), "track_id": int(s["track_id"]), "first_frame": int(s["first_frame"]),
                        "last_frame": int(s["last_frame"]), "hits": int(s["hits"]), "cls": int(s["voted_class"]), "cls_conf": float(s["voted_conf"]),
                        "bbox": tuple(int(v) for v in (s["x1"], s["y1"], s["x2"], s["y2"])), "det_class": int(s["det_class"]),
                        "best_frame": int(s["best_frame"]), "crop": wc[i] if s["flags"] & V.HAS_CROP else None,
                        "flushed": bool(s["flags"] & V.FLUSHED)} for i, s in enumerate(ws)), key=key)
        n_crops = 0
        for g, w in zip(sorted(got, key=key), want):
            assert {k: v for k, v in g.items() if k != "crop"} == {k: v for k, v in w.items() if k != "crop"}
            assert (g["crop"] is None) == (w["crop"] is None)
            if g["crop"] is not None:
                assert g["crop"].shape == (S, S, 3) and g["crop"].tobytes() == w["crop"].tobytes()
                n_crops += 1
        assert n_crops >= 1 and pipe.signs_dropped == 0
    finally:
        pipe.close()
    pipe = HybridPipeline(p, b, models["cls_file"], "shufflenetv2", track=True, **kw)
    try:
        with pytest.raises(ValueError, match="inventory"):
            pipe.drain_signs()
    finally:
        pipe.close()


def test_e2e_inventory_writes_signs_csv_and_crops(models, clips, tmp_path, capsys):
    from PIL import Image

    from litepi import e2e
    p, b = models["v1"]
    clip = np.concatenate([clips["nv12"][0][:2], clips["nv12"][0][:2], clips["nv12"][1][:2], clips["nv12"][1][:2]])   # 8 frames
    clip.tofile(tmp_path / "clip.nv12")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(91)}))
    out = tmp_path / "out"
    argv = ["--detector_param", p, "--detector_bin", b, "--classifier", models["cls_file"], "--clf_arch", "shufflenetv2", "--labels", str(tmp_path),
            "--classes", str(classes), "--batch_images", "3", "--max_det", "300", "--raw_frames", str(tmp_path / "clip.nv12"), "--frame_size",
            "640x640", "--pixel_format", "nv12", "--output", str(out), "--track", "--track_iou", "0.4", "--track_max_age", "0",
            "--track_min_hits", "1", "--inventory", "--inventory_best", "det_conf", "--benchmark_conf", "0.25", "--yolo_conf", "0.2", "--warmup", "2"]
    assert e2e.main(argv) == 0
    text = capsys.readouterr().out
    run = out / "v1+shufflenetv2"
    with open(run / "signs.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == e2e.SIGNS_CSV_COLUMNS and len(rows) > 3
    with open(run / "tracks.csv", newline="") as f:
        tracks = list(csv.reader(f))[1:]
    # one row per track id of tracks.csv (min_hits = 1: every track is logged, by its end or by the final flush)
    ids = sorted(int(r[1]) for r in rows[1:])
    assert ids == sorted({int(r[1]) for r in tracks if int(r[1]) > 0})
    assert f"Inventory: {len(ids)} signs" in text
    last = {}
    for r in tracks:
        if int(r[1]) > 0:
            last[int(r[1])] = r
    n_png = 0
    for r in rows[1:]:
        rec = dict(zip(e2e.SIGNS_CSV_COLUMNS, r))
        lt = last[int(rec["track_id"])]
        assert (int(rec["last_frame"]), int(rec["hits"]), int(rec["voted_class"])) == (int(lt[0]), int(lt[11]), int(lt[9]))
        assert int(rec["first_frame"]) <= int(rec["best_frame"]) <= int(rec["last_frame"])
        if rec["crop"]:
            im = np.asarray(Image.open(run / rec["crop"]))
            assert im.shape == (S, S, 3)
            n_png += 1
    assert n_png >= 1 and any(int(dict(zip(e2e.SIGNS_CSV_COLUMNS, r))["flushed"]) for r in rows[1:])
