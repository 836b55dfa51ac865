"""GPU tests of sign tracking (include/litepi.h, lp_track_*): the device tracker against the NumPy restatement of the rule
(tests/tracking_ref.py).  Every comparison is exact: integers equal, floats bit-equal (same operations in the same order,
nothing contracted).

1. rule: lp_track on synthetic record streams == the oracle, field for field, snapshot and accumulators included;
2. the result does not depend on how a sequence is split into calls;
3. streams do not interact;
4. lp_track_device behind lp_run_batch_device / lp_run_tiled_device / NV12 input, several calls deep without a synchronise,
   == lp_track on the downloaded records;
5. a tracker that is not used changes nothing;
6. argument errors; 7. reset and re-create; 8. HybridPipeline(track=True) and e2e --track."""
import csv
import itertools
import json

import numpy as np
import pytest
import torch

import pixfmt_ref as P
import tracking_ref as R

pytestmark = pytest.mark.gpu

NC = 58
MARGIN = 1e-4


# ---------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def engines():
    """handles without models (lp_track needs none), keyed by max_det"""
    from litepi import Engine
    es = {md: Engine(precision="fp16", max_batch=64, max_det=md, num_classes=NC) for md in (16, 300)}
    yield es
    for e in es.values():
        e.close()


def assert_records_equal(got, want, counts, tag):
    for b, n in enumerate(counts):
        g, w = got[b, :n], want[b, :n]
        if g.tobytes() != w.tobytes():
            for name in g.dtype.names:
                bad = np.flatnonzero(g[name].view(np.int32) != w[name].view(np.int32))
                assert len(bad) == 0, f"{tag}: frame {b}, field {name}, record {bad[0]}: got {g[name][bad[0]]!r}, want {w[name][bad[0]]!r}"


def assert_snapshot_equal(got, want, tag):
    assert got["next_id"] == want["next_id"] and got["overflow"] == want["overflow"], \
        f"{tag}: next_id / overflow {got['next_id']} / {got['overflow']} vs {want['next_id']} / {want['overflow']}"
    g, w = got["tracks"], want["tracks"]
    assert len(g) == len(w), f"{tag}: {len(g)} live tracks, want {len(w)}"
    for name in g.dtype.names:
        bad = np.flatnonzero(g[name].view(np.int32) != w[name].view(np.int32))
        assert len(bad) == 0, f"{tag}: snapshot field {name}, track {bad[0]}: got {g[name][bad[0]]!r}, want {w[name][bad[0]]!r}"
    assert got["acc"].shape == want["acc"].shape and got["acc"].tobytes() == want["acc"].tobytes(), f"{tag}: vote accumulators differ"


def run_calls(eng, dets, counts, chunk, stream_ids=None):
    outs = []
    for i in range(0, len(counts), chunk):
        outs.append(eng.track(dets[i:i + chunk], counts[i:i + chunk], None if stream_ids is None else stream_ids[i:i + chunk]))
    return np.concatenate(outs, 0)


# ---------------------------------------------------------------------------- 1. the rule
RULE_CONFIGS = [dict(motion=m, class_gate=g, vote_decay=d, max_age=a, min_hits=h, max_tracks=t, max_det=md)
                for m, g, d, a, h, t, md in itertools.product((0, 1), (0, 1), (1.0, 0.9), (0, 3), (1, 3), (4, 256), (16, 300))]
# one scene per configuration; the seeds were chosen on the CPU (the first of 1000 * k + 0, 1, .. whose oracle run keeps every
# match decision at least MARGIN away from flipping) and are constants: no scene is skipped or re-drawn at run time
RULE_SEEDS = [
    0, 1000, 2000, 3000, 4000, 5000, 6000, 7000, 8000, 9000, 10000, 11000, 12000, 13000, 14000, 15000,
    16000, 17000, 18000, 19000, 20000, 21000, 22000, 23000, 24000, 25000, 26000, 27000, 28000, 29000, 30001, 31000,
    32000, 33000, 34000, 35000, 36000, 37000, 38000, 39000, 40000, 41000, 42000, 43000, 44000, 45000, 46000, 47000,
    48000, 49000, 50000, 51000, 52000, 53000, 54000, 55000, 56000, 57000, 58000, 59000, 60000, 61000, 62000, 63000,
    64000, 65000, 66000, 67000, 68000, 69000, 70000, 71000, 72000, 73000, 74000, 75000, 76000, 77000, 78000, 79000,
    80000, 81000, 82001, 83000, 84000, 85000, 86000, 87000, 88000, 89000, 90000, 91000, 92000, 93000, 94000, 95000,
    96000, 97000, 98000, 99000, 100000, 101000, 102000, 103000, 104000, 105000, 106000, 107000, 108000, 109000, 110000, 111000,
    112000, 113000, 114000, 115000, 116000, 117000, 118000, 119000, 120000, 121000, 122000, 123000, 124000, 125000, 126000, 127000,
]


def rule_id(k):
    c = RULE_CONFIGS[k]
    return f"{k}-m{c['motion']}g{c['class_gate']}d{c['vote_decay']}a{c['max_age']}h{c['min_hits']}t{c['max_tracks']}md{c['max_det']}"


@pytest.mark.parametrize("k", range(len(RULE_CONFIGS)), ids=rule_id)
def test_rule_equals_oracle(engines, k):
    cfg = dict(RULE_CONFIGS[k])
    md = cfg.pop("max_det")
    dets, counts = R.make_scene(RULE_SEEDS[k], max_det=md, num_classes=NC)
    assert 40 <= len(counts) <= 200
    ref = R.TrackerRef(max_det=md, num_classes=NC, **cfg)
    want = ref.track(dets, counts)
    assert ref.min_margin >= MARGIN, f"scene {RULE_SEEDS[k]}: a match decision has margin {ref.min_margin:.3g}"
    eng = engines[md]
    eng.tracker_create(**cfg)
    got = run_calls(eng, dets, counts, 32)
    assert_records_equal(got, want, counts, rule_id(k))
    assert_snapshot_equal(eng.tracker_snapshot(0), ref.snapshot(0), rule_id(k))
    if cfg["max_tracks"] == 4 and counts.max() > 4:
        assert ref.snapshot(0)["overflow"] > 0, "the small table must overflow"


def test_rule_ties_and_large_frames(engines):
    """exact ties (identical boxes, equal scores, equal votes) and frames beyond the LDS record cache: no margin here, the
    arithmetic is the same on both sides"""
    rng = np.random.default_rng(17)
    md = 300
    T = 40
    dets = np.zeros((T, md), dtype=R.DET_DTYPE)
    counts = np.full(T, md, np.int32)
    counts[5] = 0
    counts[9] = 77
    gx, gy = np.meshgrid(np.arange(20), np.arange(15))
    for t in range(T):
        x1 = (gx.ravel() * 60 + 2 * t).astype(np.float32)
        y1 = (gy.ravel() * 45).astype(np.float32)
        d = dets[t]
        d["x1"], d["y1"], d["x2"], d["y2"] = x1, y1, x1 + 40, y1 + 30
        d["det_conf"] = rng.choice(np.array([0.3, 0.5, 0.5, 0.7], np.float32), md)   # many equal scores
        d["det_class"] = rng.integers(0, 2, md)
        d["cls_class"] = rng.integers(-1, 3, md)
        d["cls_conf"] = np.float32(0.5)
        d[10:14] = d[10]   # four identical records
        dets[t] = d[rng.permutation(md)]
    for cfg in (dict(max_tracks=256, motion=1), dict(max_tracks=256, motion=0, class_gate=0, vote_decay=0.9, max_age=1), dict(max_tracks=64)):
        ref = R.TrackerRef(max_det=md, num_classes=NC, **cfg)
        want = ref.track(dets, counts)
        engines[md].tracker_create(**cfg)
        got = run_calls(engines[md], dets, counts, 16)
        assert_records_equal(got, want, counts, str(cfg))
        assert_snapshot_equal(engines[md].tracker_snapshot(0), ref.snapshot(0), str(cfg))
        assert ref.snapshot(0)["overflow"] > 0


def test_keep_all_handle_uses_the_scratch_path():
    """max_det = 8400 (keep-all) with a frame of more detections than the in-LDS key table holds"""
    from litepi import Engine
    md, n = 8400, 1500
    rng = np.random.default_rng(23)
    dets = np.zeros((3, md), dtype=R.DET_DTYPE)
    counts = np.array([n, 40, n], np.int32)
    for t in range(3):
        i = np.arange(md)
        d = dets[t]
        d["x1"], d["y1"] = ((i % 100) * 30 + t).astype(np.float32), ((i // 100) * 30).astype(np.float32)
        d["x2"], d["y2"] = d["x1"] + 20, d["y1"] + 20
        d["det_conf"] = rng.uniform(0.25, 1.0, md).astype(np.float32)
        d["cls_class"], d["cls_conf"] = rng.integers(0, NC, md), rng.uniform(0.2, 1.0, md).astype(np.float32)
    e = Engine(precision="fp16", max_batch=4, max_det=md, num_classes=NC)
    try:
        cfg = dict(max_tracks=256, max_age=2)
        e.tracker_create(**cfg)
        ref = R.TrackerRef(max_det=md, num_classes=NC, **cfg)
        want = ref.track(dets, counts)
        got = e.track(dets, counts)
        assert_records_equal(got, want, counts, "keep-all")
        assert_snapshot_equal(e.tracker_snapshot(0), ref.snapshot(0), "keep-all")
    finally:
        e.close()


# ---------------------------------------------------------------------------- 2. batch-split invariance
def test_batch_split_invariance(engines):
    cfg = dict(max_tracks=32, max_age=3, vote_decay=0.9)
    dets, counts = R.make_scene(4242, max_det=16, num_classes=NC, n_frames=64, n_signs=12)
    ref = R.TrackerRef(max_det=16, num_classes=NC, **cfg)
    want = ref.track(dets, counts)
    eng = engines[16]
    for chunk in (1, 64, 7):
        eng.tracker_create(**cfg)
        got = run_calls(eng, dets, counts, chunk)
        assert_records_equal(got, want, counts, f"B = {chunk}")
        assert_snapshot_equal(eng.tracker_snapshot(0), ref.snapshot(0), f"B = {chunk}")


# ---------------------------------------------------------------------------- 3. stream independence
def test_interleaved_streams_equal_each_sequence_alone(engines):
    cfg = dict(max_tracks=16, max_age=2)
    eng = engines[16]
    scenes = [R.make_scene(s, max_det=16, num_classes=NC, n_frames=21, n_signs=6) for s in (501, 502, 503)]
    sids = [4, 0, 2]
    rng = np.random.default_rng(8)
    order = rng.permutation(np.repeat(np.arange(3), 21))   # an arbitrary interleaving that keeps each sequence's own order
    pos = [0, 0, 0]
    dets = np.zeros((63, 16), dtype=R.DET_DTYPE)
    counts = np.zeros(63, np.int32)
    where = [[], [], []]
    for b, q in enumerate(order):
        dets[b], counts[b] = scenes[q][0][pos[q]], scenes[q][1][pos[q]]
        where[q].append(b)
        pos[q] += 1
    stream_ids = np.array([sids[q] for q in order], np.int32)
    eng.tracker_create(n_streams=5, **cfg)
    got = eng.track(dets, counts, stream_ids)   # one call
    snaps = [eng.tracker_snapshot(s) for s in sids]
    assert len(eng.tracker_snapshot(1)["tracks"]) == 0 and eng.tracker_snapshot(3)["next_id"] == 1
    for q in range(3):
        ref = R.TrackerRef(max_det=16, num_classes=NC, **cfg)
        want = ref.track(*scenes[q])
        assert_records_equal(got[where[q]], want, scenes[q][1], f"sequence {q} (oracle)")
        assert_snapshot_equal(snaps[q], ref.snapshot(0), f"sequence {q} (oracle)")
        eng.tracker_create(**cfg)   # the same sequence alone on the device
        alone = eng.track(*scenes[q])
        assert_records_equal(got[where[q]], alone, scenes[q][1], f"sequence {q} (alone)")


def test_64_streams_one_frame_per_call(engines):
    cfg = dict(max_tracks=8, max_age=1, n_streams=64)
    eng = engines[16]
    scenes = [R.make_scene(9000 + s, max_det=16, num_classes=NC, n_frames=40, n_signs=5) for s in range(64)]
    eng.tracker_create(**cfg)
    ref = R.TrackerRef(max_det=16, num_classes=NC, **cfg)
    sid = np.arange(64, dtype=np.int32)[::-1].copy()   # frame b of a call belongs to stream 63 - b
    for t in range(40):
        dets = np.stack([scenes[s][0][t] for s in sid])
        counts = np.array([scenes[s][1][t] for s in sid], np.int32)
        assert_records_equal(eng.track(dets, counts, sid), ref.track(dets, counts, sid), counts, f"call {t}")
    for s in (0, 17, 63):
        assert_snapshot_equal(eng.tracker_snapshot(s), ref.snapshot(s), f"stream {s}")
        alone = R.TrackerRef(max_det=16, num_classes=NC, **dict(cfg, n_streams=1))
        alone.track(*scenes[s])
        assert_snapshot_equal(eng.tracker_snapshot(s), alone.snapshot(0), f"stream {s} alone")


# ---------------------------------------------------------------------------- models of the pipeline tests
CONF, IOU, MIN_AREA = 0.25, 0.45, 50
# the repeated-frame checks ("every detection keeps its id") need a match threshold above the NMS threshold: two kept boxes of
# one class overlap by at most IOU, so with iou_match > IOU a detection can only claim the track that holds its own box and
# never the track of a neighbour that comes later in score order
STRICT_IOU = 0.5


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(77)
    base = rng.integers(0, 256, (4, 640, 640, 3), dtype=np.uint8)
    nv = [P.bgr_to_nv12(f) for f in rng.integers(0, 256, (4, 640, 640, 3), dtype=np.uint8)]
    big = rng.integers(0, 256, (2, 800, 1000, 3), dtype=np.uint8)
    return {"640": base, "nv12": np.stack(nv), "nv12_bgr": np.stack([P.nv12_to_bgr(f, "bt601") for f in nv]), "big": big}


@pytest.fixture(scope="module")
def models(tmp_path_factory, frames):
    """seeded v1 / v2 detectors whose class bias is shifted so that on every frame of the test sets at least three anchors
    pass conf 0.25 with a margin of 0.1 in the logit, measured with the device's own scores (as tests/test_gpu_pixfmt.py)"""
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    d = tmp_path_factory.mktemp("track_models")
    sd = random_shufflenet_state(91, seed=3)
    cls_file = str(d / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, cls_file)
    out = {"cls": sd, "cls_file": cls_file}
    every = list(frames["640"]) + list(frames["nv12_bgr"]) + list(frames["big"])
    for preset in ("v1", "v2"):
        p, b = str(d / f"{preset}.param"), str(d / f"{preset}.bin")
        ncnn_export.export_detector(p, b, preset, seed=4321, cls_bias=0.0)
        e = Engine(precision="fp16", max_batch=len(every), max_det=300, num_classes=91)
        try:
            e.load_detector(p, b)
            lb = np.stack([e.test_letterbox(f)[0] for f in every])
            s = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64), axis=1)[:, ::-1]
        finally:
            e.close()
        third = s[:, 2].min()
        ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - (np.log(third / (1 - third)) - 0.1)))
        out[preset] = (p, b)
    return out


def _engine(models, preset, prec, max_batch=16):
    from litepi import Engine
    e = Engine(precision=prec, max_batch=max_batch, max_det=300, num_classes=91)
    e.load_detector(*models[preset])
    e.load_classifier(models["cls"])
    return e


def _device_chain(eng, dev_inputs, launch, B, cfg, tag):
    """one pipeline call + lp_track_device per input, all enqueued without a synchronise; every frame of a call is its own
    stream.  Returns the downloaded (dets, counts, tracks) per call after checking them against lp_track on the downloaded
    records and against the oracle."""
    from litepi._ffi import DET_DTYPE, TRACK_DTYPE
    dev = torch.device("cuda", 0)
    md = eng.cfg.max_det
    n = len(dev_inputs)
    bufs = [(torch.zeros(B * md * 32, dtype=torch.uint8, device=dev), torch.zeros(3 * B, dtype=torch.int32, device=dev),
             torch.full((B * md * 32,), 0xEE, dtype=torch.uint8, device=dev)) for _ in range(n)]
    sid = np.arange(B, dtype=np.int32)
    st = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    eng.set_stream(st.cuda_stream)
    eng.tracker_create(n_streams=B, **cfg)
    with torch.cuda.stream(st):
        for x, (d, c, t) in zip(dev_inputs, bufs):
            launch(x, d.data_ptr(), c.data_ptr())
            eng.track_device(d.data_ptr(), c.data_ptr(), B, t.data_ptr(), sid)
    eng.synchronize()
    torch.cuda.synchronize()
    calls = []
    for d, c, t in bufs:
        counts = c.cpu().numpy()[:B].copy()
        dets = d.cpu().numpy().view(DET_DTYPE).reshape(B, md)
        raw = t.cpu().numpy().reshape(B, md, 32)
        for b in range(B):   # only the first count[b] records of a frame are written
            assert (raw[b, counts[b]:] == 0xEE).all(), f"{tag}: records beyond the count of frame {b} were written"
        calls.append((dets, counts, raw.reshape(-1).view(TRACK_DTYPE).reshape(B, md)))
    eng.tracker_create(n_streams=B, **cfg)   # ids restart: the host entry point on the downloaded records
    ref = R.TrackerRef(max_det=md, num_classes=91, n_streams=B, **cfg)
    for k, (dets, counts, tracks) in enumerate(calls):
        host = eng.track(dets, counts, sid)
        assert_records_equal(tracks, host, counts, f"{tag}: call {k}, device vs host entry point")
        assert_records_equal(tracks, ref.track(dets, counts, sid), counts, f"{tag}: call {k}, device vs oracle")
    eng.set_stream(0)
    return calls


def _check_repeat(prev, cur, tag):
    """cur is the call after prev on the same frames: every detection keeps its id and hits goes up by one (a detection that
    found the table full stays untracked)"""
    (d0, c0, t0), (d1, c1, t1) = prev, cur
    assert np.array_equal(c0, c1), f"{tag}: a repeated frame gave other counts"
    total = 0
    for b, n in enumerate(c0):
        assert d0[b, :n].tobytes() == d1[b, :n].tobytes(), f"{tag}: a repeated frame gave other records"
        tracked = t0[b, :n]["track_id"] > 0
        assert np.array_equal(t1[b, :n]["track_id"], t0[b, :n]["track_id"]), f"{tag}: frame {b}: ids changed on a repeated frame"
        assert np.array_equal(t1[b, :n]["hits"][tracked], t0[b, :n]["hits"][tracked] + 1), f"{tag}: frame {b}: hits did not go up by one"
        total += int(tracked.sum())
    return total


# ---------------------------------------------------------------------------- 4. device path
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("preset", ["v1", "v2"])
def test_track_device_behind_run_batch_device(models, frames, preset, prec):
    base = frames["640"]
    B = len(base)
    seq = [base, base, np.roll(base, 3, axis=2), np.roll(base, 3, axis=2)]   # repeat, shift by 3 px, repeat
    dev = torch.device("cuda", 0)
    eng = _engine(models, preset, prec)
    try:
        dev_inputs = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in seq]
        calls = _device_chain(eng, dev_inputs, lambda x, d, c: eng.run_batch_device(x.data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d, c),
                              B, dict(max_tracks=256, max_age=2, min_hits=2, motion=0, iou_match=STRICT_IOU), f"{preset} {prec}")
        n = _check_repeat(calls[0], calls[1], f"{preset} {prec}") + _check_repeat(calls[2], calls[3], f"{preset} {prec}")
        assert n >= 2 * 3 * B, f"only {n} detections on the repeated frames"
        for b, cnt in enumerate(calls[1][1]):   # min_hits = 2: every track is confirmed on its second frame
            t = calls[1][2][b, :cnt]
            assert np.array_equal((t["flags"] & 1) != 0, t["track_id"] > 0)
    finally:
        eng.close()


def test_track_device_behind_run_tiled_device(models, frames):
    big = frames["big"]
    B = len(big)
    dev = torch.device("cuda", 0)
    eng = _engine(models, "v1", "fp16")
    try:
        dev_inputs = [torch.from_numpy(big).to(dev) for _ in range(3)]
        calls = _device_chain(eng, dev_inputs, lambda x, d, c: eng.run_tiled_device(x.data_ptr(), B, 800, 1000, CONF, IOU, MIN_AREA, d, c, overlap=128),
                              B, dict(max_tracks=256, iou_match=STRICT_IOU), "tiled")
        assert _check_repeat(calls[0], calls[1], "tiled") + _check_repeat(calls[1], calls[2], "tiled") >= 2 * 3 * B
    finally:
        eng.close()


def test_track_device_with_nv12_input(models, frames):
    nv = frames["nv12"]
    B = len(nv)
    dev = torch.device("cuda", 0)
    eng = _engine(models, "v1", "fp16")
    try:
        eng.set_input_format("nv12", "bt601")
        dev_inputs = [torch.from_numpy(nv).to(dev) for _ in range(3)]
        calls = _device_chain(eng, dev_inputs, lambda x, d, c: eng.run_batch_device(x.data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d, c),
                              B, dict(max_tracks=256, iou_match=STRICT_IOU), "nv12")
        assert _check_repeat(calls[0], calls[1], "nv12") + _check_repeat(calls[1], calls[2], "nv12") >= 2 * 3 * B
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 5. no side effect
def test_unused_tracker_changes_nothing(models, frames):
    base = frames["640"]
    B = len(base)
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(base).to(dev)
    results = []
    for with_tracker in (False, True):
        eng = _engine(models, "v1", "fp16")
        try:
            if with_tracker:
                eng.tracker_create(n_streams=B, max_tracks=64)
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
            results.append((outs, launches))
        finally:
            eng.close()
    assert results[0][0] == results[1][0], "lp_run_batch_device output differs on a handle that has an unused tracker"
    assert results[0][1] == results[1][1] and len(results[0][1]) > 10, "the launch list differs on a handle that has an unused tracker"
    assert not any("track" in name for name, _ in results[1][1])


# ---------------------------------------------------------------------------- 6. errors
def test_errors_leave_the_handle_usable():
    from litepi import Engine, _ffi
    from litepi._ffi import LitepiError
    eng = Engine(precision="fp16", max_batch=4, max_det=16, num_classes=NC)
    try:
        dets, counts = R.make_scene(31, max_det=16, num_classes=NC, n_frames=8, n_signs=3)
        dev = torch.device("cuda", 0)
        d = torch.from_numpy(dets[:4].view(np.uint8).reshape(-1).copy()).to(dev)
        c = torch.from_numpy(counts[:4].copy()).to(dev)
        t = torch.zeros(4 * 16 * 32, dtype=torch.uint8, device=dev)

        def code(fn):
            with pytest.raises(LitepiError) as ei:
                fn()
            return ei.value.code

        # no tracker
        assert code(lambda: eng.track(dets[:4], counts[:4])) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.track_device(d.data_ptr(), c.data_ptr(), 4, t.data_ptr())) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.tracker_reset()) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.tracker_snapshot(0)) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.tracker_create(max_tracks=0)) == _ffi.LP_ERR_ARG
        eng.tracker_create(n_streams=2, max_tracks=8)
        ref = R.TrackerRef(max_det=16, num_classes=NC, n_streams=2, max_tracks=8)
        want = ref.track(dets[:4], counts[:4])
        assert_records_equal(eng.track(dets[:4], counts[:4]), want, counts[:4], "first valid call")
        # B > max_batch, B <= 0, stream id out of range: LP_ERR_ARG before anything is enqueued, and the tracker state is untouched
        assert code(lambda: eng.track(dets[:5], counts[:5])) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.track_device(d.data_ptr(), c.data_ptr(), 5, t.data_ptr())) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.track_device(d.data_ptr(), c.data_ptr(), 0, t.data_ptr())) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.track_device(d.data_ptr(), c.data_ptr(), -1, t.data_ptr())) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.track(dets[:4], counts[:4], [0, 1, 2, 0])) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.track(dets[:4], counts[:4], [0, -1, 0, 0])) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.track_device(d.data_ptr(), c.data_ptr(), 4, t.data_ptr(), [0, 1, 1, 2])) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.tracker_reset(2)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.tracker_snapshot(2)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.tracker_snapshot(-1)) == _ffi.LP_ERR_ARG
        assert_snapshot_equal(eng.tracker_snapshot(0), ref.snapshot(0), "after the refused calls")
        want = ref.track(dets[4:8], counts[4:8], [0, 1, 0, 1])
        assert_records_equal(eng.track(dets[4:8], counts[4:8], [0, 1, 0, 1]), want, counts[4:8], "next valid call")
        for s in (0, 1):
            assert_snapshot_equal(eng.tracker_snapshot(s), ref.snapshot(s), f"stream {s}")
        eng.tracker_destroy()
        assert not hasattr(eng, "track_cfg")
        assert code(lambda: eng.track(dets[:4], counts[:4])) == _ffi.LP_ERR_STATE
        eng.tracker_destroy()   # twice is fine
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 7. reset and re-create
def test_reset_keeps_ids_counting_and_create_restarts_them(engines):
    eng = engines[16]
    cfg = dict(n_streams=2, max_tracks=8, max_age=3)
    dets, counts = R.make_scene(77, max_det=16, num_classes=NC, n_frames=40, n_signs=6)
    eng.tracker_create(**cfg)
    ref = R.TrackerRef(max_det=16, num_classes=NC, **cfg)
    sid = np.array([0, 1] * 10, np.int32)
    assert_records_equal(eng.track(dets[:20], counts[:20], sid), ref.track(dets[:20], counts[:20], sid), counts[:20], "before the reset")
    used = ref.snapshot(1)["next_id"]
    assert used > 1
    eng.tracker_reset(1)
    ref.reset(1)
    snap = eng.tracker_snapshot(1)
    assert len(snap["tracks"]) == 0 and snap["next_id"] == used
    assert_snapshot_equal(eng.tracker_snapshot(0), ref.snapshot(0), "stream 0 is not reset")
    got = eng.track(dets[20:40], counts[20:40], sid)
    assert_records_equal(got, ref.track(dets[20:40], counts[20:40], sid), counts[20:40], "after the reset")
    ids1 = np.concatenate([got[b, :counts[20 + b]]["track_id"] for b in range(1, 20, 2)])
    assert ids1[ids1 > 0].min() >= used, "an id was reused after lp_tracker_reset"
    eng.tracker_reset(-1)
    ref.reset(-1)
    for s in (0, 1):
        assert_snapshot_equal(eng.tracker_snapshot(s), ref.snapshot(s), f"reset of all streams, stream {s}")
    eng.tracker_create(**cfg)
    f = int(np.flatnonzero(counts > 0)[0])   # the first frame that holds a detection: all of them are born, in record order
    first = eng.track(dets[f:f + 1], counts[f:f + 1])[0, :counts[f]]["track_id"]
    assert first.tolist() == list(range(1, counts[f] + 1)), "ids restart at 1 after lp_tracker_create"


# ---------------------------------------------------------------------------- 8. Python and CLI
TRACK_KEYS = ("track_id", "track_hits", "track_age", "track_cls", "track_cls_conf", "track_confirmed")


@pytest.mark.parametrize("mode", ["plain", "tiled", "nv12"])
def test_hybrid_pipeline_track(models, frames, mode):
    from litepi import HybridPipeline
    p, b = models["v1"]
    kw = dict(num_classes=91, precision="fp16", max_batch=16, max_det=300)
    if mode == "plain":
        seq = [list(frames["640"]), list(frames["640"]), list(np.roll(frames["640"], 3, axis=2))]
    elif mode == "tiled":
        kw["tile_overlap"] = 128
        seq = [list(frames["big"])] * 3
    else:
        kw["pixel_format"] = "nv12"
        seq = [list(frames["nv12"])] * 3
    B = len(seq[0])
    tcfg = dict(n_streams=B, max_tracks=256, min_hits=2, iou_match=STRICT_IOU)
    sid = list(range(B))
    pipe = HybridPipeline(p, b, models["cls_file"], "shufflenetv2", track=True, track_config=tcfg, **kw)
    try:
        ref = R.TrackerRef(max_det=300, num_classes=91, **tcfg)
        total = 0
        for k, imgs in enumerate(seq):
            got = pipe.run_batch(imgs, CONF, IOU, MIN_AREA, stream_ids=sid)
            plain = pipe.run_batch(imgs, CONF, IOU, MIN_AREA, track=False)   # not tracked: the tracker is not fed, no new key
            dets, counts, _, _ = (pipe._run_tiled(imgs, CONF, IOU, MIN_AREA) if mode == "tiled" else pipe.engine.run_batch(imgs, CONF, IOU, MIN_AREA))
            want = ref.track(dets, counts.astype(np.int32), sid)
            for i in range(B):
                res, res_plain = got[i][0], plain[i][0]
                assert len(res) == counts[i] == len(res_plain)
                for j, (r, q) in enumerate(zip(res, res_plain)):
                    assert not any(key in q for key in TRACK_KEYS), "track=False result dicts must not gain a key"
                    assert {key: v for key, v in r.items() if key not in TRACK_KEYS and not key.startswith("time_")} == \
                           {key: v for key, v in q.items() if not key.startswith("time_")}
                    w = want[i, j]
                    assert (r["track_id"], r["track_hits"], r["track_age"], r["track_cls"], r["track_confirmed"]) == \
                           (w["track_id"], w["hits"], w["age"], w["voted_class"], bool(w["flags"] & 1)), (mode, k, i, j)
                    assert np.float32(r["track_cls_conf"]) == w["voted_conf"]
                    if k == 1 and r["track_id"] > 0:
                        assert r["track_hits"] == 2 and r["track_confirmed"]
                    total += 1
        assert total >= 3 * 3 * B
    finally:
        pipe.close()
    pipe = HybridPipeline(p, b, models["cls_file"], "shufflenetv2", **kw)
    try:
        assert not any(key in r for res, _ in pipe.run_batch(seq[0], CONF, IOU, MIN_AREA) for r in res for key in TRACK_KEYS)
        with pytest.raises(ValueError, match="track"):
            pipe.run_batch(seq[0], CONF, IOU, MIN_AREA, track=True)
    finally:
        pipe.close()


def test_e2e_track_writes_tracks_csv(models, frames, tmp_path, capsys):
    from litepi import HybridPipeline, e2e
    p, b = models["v1"]
    clip = np.concatenate([frames["nv12"], frames["nv12"][:2], frames["nv12"][:2]])   # 8 frames; the last four repeat two
    clip.tofile(tmp_path / "clip.nv12")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(91)}))
    out = tmp_path / "out"
    argv = ["--detector_param", p, "--detector_bin", b, "--classifier", models["cls_file"], "--clf_arch", "shufflenetv2", "--labels", str(tmp_path),
            "--classes", str(classes), "--batch_images", "3", "--max_det", "300", "--raw_frames", str(tmp_path / "clip.nv12"), "--frame_size",
            "640x640", "--pixel_format", "nv12", "--output", str(out), "--track", "--track_iou", "0.4", "--track_max_age", "1",
            "--track_min_hits", "2", "--benchmark_conf", "0.25", "--yolo_conf", "0.2", "--warmup", "2"]   # the warm-up frames must not reach the tracker
    assert e2e.main(argv) == 0
    text = capsys.readouterr().out
    with open(out / "v1+shufflenetv2" / "tracks.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == e2e.TRACKS_CSV_COLUMNS
    # the oracle on the same pipeline's records, frame by frame at the benchmark threshold
    pipe = HybridPipeline(p, b, models["cls_file"], "shufflenetv2", num_classes=91, precision="fp16", max_batch=3, max_det=300, pixel_format="nv12")
    try:
        ref = R.TrackerRef(max_det=300, num_classes=91, iou_match=0.4, max_age=1, min_hits=2)
        want = []
        for i in range(0, 8, 3):
            dets, counts, _, _ = pipe.engine.run_batch(list(clip[i:i + 3]), 0.25, 0.45, 50)
            tr = ref.track(dets, counts.astype(np.int32))
            for k in range(len(counts)):
                for d, t in zip(dets[k, :counts[k]], tr[k, :counts[k]]):
                    want.append([i + k, int(t["track_id"]), int(d["x1"]), int(d["y1"]), int(d["x2"]), int(d["y2"]), float(d["det_conf"]),
                                 int(d["cls_class"]), float(d["cls_conf"]), int(t["voted_class"]), float(t["voted_conf"]), int(t["hits"]),
                                 int(bool(t["flags"] & 1))])
    finally:
        pipe.close()
    got = [[int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), int(r[5]), float(r[6]), int(r[7]), float(r[8]), int(r[9]), float(r[10]),
            int(r[11]), int(r[12])] for r in rows[1:]]
    assert len(got) >= 8 * 3 and got == want
    confirmed = len({r[1] for r in want if r[12] and r[1] > 0})
    assert confirmed > 0 and f"Tracking: {confirmed} confirmed tracks" in text
