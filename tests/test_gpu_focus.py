"""GPU tests of focus views (lp_focus_*, lp_run_focus, lp_run_focus_device):

1. the device plan equals the NumPy rule (tests/focus_ref.py) int for int, cursor and unserved included, on a det_input 64
   handle without models: the tracker is seeded with lp_track on crafted records, the rule reads lp_tracker_snapshot;
2. the pipeline behind the plan equals scaled views: every frame's records, counts and windows are byte-equal to
   lp_run_views_device on the whole frame + the windows the plan chose (models of tests/test_gpu_views.py, det_input 320);
3. the captured step keeps replaying while the windows move; 4. tracker, inventory, errors, HybridPipeline and the CLI.

The frame NMS capacity (LP_ERR_ARG of the shared layout builder) cannot be reached here: 1 + 16 views of a frame stay far
below it at every det_input the detector takes; tests/test_gpu_tiling.py covers that refusal of the builder."""
import csv
import json

import numpy as np
import pytest
import torch

import focus_ref as R
from test_gpu_views import CONF, H, IOU, MIN_AREA, S, W, _engine, make_models

pytestmark = pytest.mark.gpu

NC = 58


# ---------------------------------------------------------------------------- 1. the rule
def _records(max_det, boxes):
    from litepi._ffi import DET_DTYPE
    d = np.zeros((1, max_det), dtype=DET_DTYPE)
    n = len(boxes)
    for k, name in enumerate(("x1", "y1", "x2", "y2")):
        d[name][0, :n] = boxes[:, k]
    d["det_conf"][0, :n] = 0.9
    d["cls_class"][0, :n] = -1
    return d, np.array([n], np.int32)


def seed(eng, stream, frames_boxes):
    for boxes in frames_boxes:
        d, c = _records(eng.cfg.max_det, np.asarray(boxes, np.float32).reshape(-1, 4))
        eng.track(d, c, [stream])


def scene(rng, n, fh, fw, nan_at=None):
    """three frames of n boxes moving by a constant step; the second half is born one frame later (fewer hits)"""
    c = np.stack([rng.uniform(-10, fw + 10, n), rng.uniform(-10, fh + 10, n)], 1)
    half = np.stack([rng.uniform(1.5, 22, n), rng.uniform(1.5, 22, n)], 1)
    step = rng.integers(-12, 13, (n, 2)) * 0.25
    out = []
    for f in range(3):
        m = n if f > 0 else max(1, n // 2)
        cf = c + f * step
        b = np.concatenate([cf - half, cf + half], 1).astype(np.float32)[:m]
        if nan_at is not None and nan_at < m:
            b[nan_at, 2] = np.nan
        out.append(b)
    return out


RULE = [dict(T=1, slots=1), dict(T=64, slots=3), dict(T=64, slots=1, sweep=0, motion=0), dict(T=256, slots=16),
        dict(T=256, slots=3, sweep=0, border=0, margin=3.5, small_px=9.0),
        dict(T=64, slots=16, motion=0, side_min=48, side_max=200, sweep_overlap=16, nan_at=3)]


@pytest.fixture(scope="module")
def rule_engine():
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=64, max_det=300, num_classes=NC, det_input=64)
    yield e
    e.close()


@pytest.mark.parametrize("k", range(len(RULE)))
def test_plan_equals_the_numpy_rule(rule_engine, k):
    eng = rule_engine
    cfg = dict(RULE[k])
    T, motion, nan_at = cfg.pop("T"), cfg.pop("motion", 1), cfg.pop("nan_at", None)
    rng = np.random.default_rng(100 + k)
    eng.tracker_create(n_streams=2, max_tracks=T, motion=motion, max_age=3)
    seed(eng, 0, scene(rng, T, 200, 264, nan_at))
    seed(eng, 1, scene(rng, min(T, 5), 200, 264))
    eng.focus_create(**cfg)
    snaps = {s: eng.tracker_snapshot(s)["tracks"] for s in (0, 1)}
    assert len(snaps[0]) == T, "not every slot of stream 0 is live"
    if motion and T > 1:   # (the single track of T = 1 may have lost its detection: it coasts)
        assert np.abs(snaps[0]["vx1"]).max() > 0 and np.abs(snaps[0]["vy1"]).max() > 0, "no track moves"
    ref = R.FocusRef(64, n_streams=2, motion=motion, **cfg)
    # two streams interleaved, three frames of stream 0 (the j rule), three frame sizes, one no larger than side_min
    ids = [0, 1, 0, 1, 0, 1]
    hs, ws = [200, 200, 120, 200, 200, 48], [264, 264, 150, 264, 264, 40]
    asked = 0
    for call in range(6):
        if call == 3:   # advance = 0, twice: the same plan, the state untouched
            before = [eng.focus_state(s) for s in (0, 1)]
            a = eng.focus_plan(hs, ws, ids, advance=False)
            b = eng.focus_plan(hs, ws, ids, advance=False)
            want = ref.plan(snaps, hs, ws, ids, advance=False)
            assert np.array_equal(a, b) and np.array_equal(a, want)
            assert [eng.focus_state(s) for s in (0, 1)] == before == ref.state
        got = eng.focus_plan(hs, ws, ids)
        want = ref.plan(snaps, hs, ws, ids)
        assert got.shape == want.shape == (6, ref.slots, 4)
        assert np.array_equal(got, want), f"call {call}: first difference at {np.argwhere(got != want)[0].tolist()}\n{got[got != want]}\n{want[got != want]}"
        assert [eng.focus_state(s) for s in (0, 1)] == ref.state, f"call {call}"
        asked += sum(len(ref.askers(snaps[s], 0, 200, 264)) for s in (0, 1))
    assert asked > 0, "no track asked for a window"
    if cfg["slots"] <= 3 and T > 1:
        assert ref.state[0]["unserved"] > 0, "no asker was left unserved"
    if cfg.get("sweep", 1) and cfg["slots"] == 16:   # (with few slots the askers may take them all: nothing is left to sweep)
        assert ref.state[0]["cursor"] != 0 or ref.state[1]["cursor"] != 0
    if nan_at is not None:
        assert np.isnan(snaps[0]["x2"]).any(), "the NaN box did not reach the table"


# ---------------------------------------------------------------------------- 2. the pipeline against scaled views
@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return make_models(tmp_path_factory.mktemp("focus"))


FCFG = dict(side_min=320, sweep_overlap=64)


def variants(models):
    """the frame the models were calibrated on, and two shifted copies of it"""
    f = models["frames"][1]
    return [f, np.ascontiguousarray(np.roll(f, 16, axis=1)), np.ascontiguousarray(np.roll(f, 32, axis=0))]


TRACKS_A = [[(100, 100, 140, 140), (600, 400, 650, 440)], [(104, 102, 144, 142), (600, 400, 650, 440)]]   # two frames: one track moves


class Dev:
    """device buffers of one comparison: frames, records, counts, windows"""

    def __init__(self, eng, frames, slots):
        self.B = len(frames)
        self.img = torch.from_numpy(np.stack(frames)).cuda()
        self.dd = torch.zeros(self.B * eng.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        self.dc = torch.zeros(3 * self.B, dtype=torch.int32, device="cuda")
        self.dv = torch.full((self.B * slots * 4,), -7, dtype=torch.int32, device="cuda")
        self.slots = slots
        torch.cuda.synchronize()

    def result(self, eng):
        from litepi._ffi import DET_DTYPE
        eng.synchronize()
        cnt = self.dc.cpu().numpy().copy()
        recs = self.dd.cpu().numpy().view(DET_DTYPE).reshape(self.B, -1).copy()
        return recs, cnt, self.dv.cpu().numpy().reshape(self.B, self.slots, 4).copy()


def run_focus(eng, dev, ids, H_=H, W_=W):
    eng.run_focus_device(dev.img.data_ptr(), dev.B, H_, W_, CONF, IOU, MIN_AREA, dev.dd.data_ptr(), dev.dc.data_ptr(), stream_ids=ids,
                         dev_views=dev.dv.data_ptr())
    return dev.result(eng)


def run_views(eng, img, B, views):
    from litepi._ffi import DET_DTYPE
    dd = torch.zeros(B * eng.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    eng.run_views_device(img.data_ptr(), B, H, W, views, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
    eng.synchronize()
    return dd.cpu().numpy().view(DET_DTYPE).reshape(B, -1), dc.cpu().numpy()


def same_frame(got, gi, B, ref, ri, RB, tag):
    """frame gi of a B-frame result equals frame ri of an RB-frame one: the three count words and the kept records"""
    (recs, cnt, _), (rrecs, rcnt) = got, ref
    words = [int(cnt[k * B + gi]) for k in range(3)], [int(rcnt[k * RB + ri]) for k in range(3)]
    assert words[0] == words[1], f"{tag}: count words {words[0]} vs {words[1]}"
    n = words[0][0]
    assert words[0][1] >= 1, f"{tag}: the frame keeps no detection, the comparison is empty"
    assert recs[gi, :n].tobytes() == rrecs[ri, :n].tobytes(), f"{tag}: records differ"


def windows(v):
    return [tuple(int(x) for x in w) for w in v if w[2] > 0]


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_focus_equals_scaled_views_three_streams(models, prec):
    """(a) identical tracks in three streams, no empty slot; eager, captured, replayed while the sweep moves the third window"""
    frames = variants(models)
    e = _engine(models, prec, 12)
    try:
        e.tracker_create(n_streams=3, max_tracks=16)
        for s in range(3):
            seed(e, s, TRACKS_A)
        e.focus_create(slots=3, **FCFG)
        dev = Dev(e, frames, 3)
        calls = []
        for call in range(3):
            plan = e.focus_plan([H] * 3, [W] * 3, [0, 1, 2], advance=False)
            got = run_focus(e, dev, [0, 1, 2])
            assert np.array_equal(got[2], plan), f"call {call}: dev_views differ from the plan"
            assert np.array_equal(plan[0], plan[1]) and np.array_equal(plan[0], plan[2]) and len(windows(plan[0])) == 3
            calls.append(got)
        assert len({c[2].tobytes() for c in calls}) == 3, "the sweep did not move the windows between the calls"
        assert windows(calls[0][2][0])[:2] == [(0, 0, 320, 320), (465, 260, 320, 320)]   # side_min windows around the two boxes
        for call, got in enumerate(calls):
            ref = run_views(e, dev.img, 3, ["full"] + windows(got[2][0]))
            for i in range(3):
                same_frame(got, i, 3, ref, i, 3, f"{prec} call {call} frame {i}")
    finally:
        e.close()


def _mixed_states(e):
    """stream 0: three far-apart small tracks (no empty slot with slots = 3), stream 1: one, stream 2: none"""
    e.tracker_create(n_streams=3, max_tracks=16)
    seed(e, 0, [[(100, 100, 140, 140), (600, 400, 650, 440), (300, 600, 330, 640)]] * 2)
    seed(e, 1, [[(700, 80, 760, 130)]] * 2)
    e.focus_create(slots=3, sweep=0, **FCFG)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_focus_equals_scaled_views_per_frame_with_empty_slots(models, prec):
    """(b) and (d): streams in different states; a frame whose slots are all empty gives lp_run_batch_device's result"""
    frames = variants(models)
    e = _engine(models, prec, 12)
    try:
        _mixed_states(e)
        dev = Dev(e, frames, 3)
        for call in range(2):
            got = run_focus(e, dev, [0, 1, 2])
            assert [len(windows(v)) for v in got[2]] == [3, 1, 0]
            assert np.array_equal(got[2], e.focus_plan([H] * 3, [W] * 3, [0, 1, 2], advance=False))
            for i in range(3):
                ref = run_views(e, dev.img[i:i + 1], 1, ["full"] + windows(got[2][i]))
                same_frame(got, i, 3, ref, 0, 1, f"{prec} call {call} frame {i}")
        # (d) no tracks at all, sweep off: every slot of every frame is empty
        e.tracker_reset(-1)
        dev = Dev(e, [frames[0]] * 3, 3)   # (of the three frames only this one keeps a detection in its whole-frame view alone)
        got = run_focus(e, dev, [0, 1, 2])
        assert not got[2].any()
        from litepi._ffi import DET_DTYPE
        dd = torch.zeros_like(dev.dd)
        dc = torch.zeros_like(dev.dc)
        e.run_batch_device(dev.img.data_ptr(), 3, H, W, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
        e.synchronize()
        ref = dd.cpu().numpy().view(DET_DTYPE).reshape(3, -1), dc.cpu().numpy()
        for i in range(3):
            same_frame(got, i, 3, ref, i, 3, f"{prec} all slots empty, frame {i}")
    finally:
        e.close()


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_focus_host_path_equals_device_path(models, fmt):
    """(c) lp_run_focus on host frames equals lp_run_focus_device"""
    import pixfmt_ref as P
    frames = variants(models)
    if fmt == "nv12":
        frames = [P.bgr_to_nv12(f) for f in frames]
    e = _engine(models, "fp16", 12)
    try:
        e.set_input_format(fmt)
        _mixed_states(e)
        dev = Dev(e, frames, 3)
        for call in range(3):
            d, c, nd, _, views = e.run_focus(frames, CONF, IOU, MIN_AREA, stream_ids=[0, 1, 2])
            avg = e.last_det_conf_avg.copy()
            got = run_focus(e, dev, [0, 1, 2])
            assert np.array_equal(views, got[2]) and [len(windows(v)) for v in views] == [3, 1, 0]
            host = (d, np.concatenate([c.astype(np.int32), nd.astype(np.int32), avg.view(np.int32)]))
            for i in range(3):
                same_frame(got, i, 3, host, i, 3, f"{fmt} call {call} frame {i}")
    finally:
        e.close()


# ---------------------------------------------------------------------------- 3. the captured step under moving windows
def test_captured_step_follows_the_moving_windows(models):
    f0, f1 = variants(models)[:2]
    e = _engine(models, "fp16", 4)
    try:
        e.tracker_create(n_streams=1, max_tracks=16, max_age=1)
        e.focus_create(slots=3, **FCFG)
        devs = [Dev(e, [f0], 3), Dev(e, [f1], 3)]
        box = np.array([[300, 200, 340, 240]], np.float32)
        calls = []
        for call in range(7):
            seed(e, 0, [box + 8 * call])   # the host feed: the track moves 8 pixels a frame
            plan = e.focus_plan([H], [W], advance=False)
            dev = devs[call % 2]
            # the same two buffers, thresholds and geometry from the third call on: the step replays, only the tables change
            got = run_focus(e, dev, None)
            assert np.array_equal(got[2], plan), f"call {call}"
            calls.append((dev, got))
        wins = [windows(g[2][0]) for _, g in calls]
        assert all(len(w) == 3 for w in wins) and len({tuple(w) for w in wins}) == 7, "the windows did not change on every call"
        assert len({w[0] for w in wins}) >= 5, "the tracked window did not move"
        for call, (dev, got) in enumerate(calls):
            ref = run_views(e, dev.img, 1, ["full"] + wins[call])
            same_frame(got, 0, 1, ref, 0, 1, f"call {call}")
    finally:
        e.close()


# ---------------------------------------------------------------------------- 4. neighbours
def test_unused_plan_changes_nothing_and_errors_leave_the_handle_usable(models):
    from litepi._ffi import LP_ERR_ARG, LP_ERR_STATE, LitepiError
    f0, f1 = variants(models)[:2]
    e = _engine(models, "fp16", 8)
    try:
        dev = Dev(e, [f0, f1], 3)
        views = ["full", (100, 40, 640, 600)]

        def batch():
            e.run_batch_device(dev.img.data_ptr(), 2, H, W, CONF, IOU, MIN_AREA, dev.dd.data_ptr(), dev.dc.data_ptr())
            r = dev.result(e)
            return r[0].tobytes(), r[1].tobytes()

        def viewed():
            r = run_views(e, dev.img, 2, views)
            return r[0].tobytes(), r[1].tobytes()

        def refused(code, fn, *a, **kw):
            with pytest.raises(LitepiError) as ex:
                fn(*a, **kw)
            assert ex.value.code == code, ex.value

        dev.dd.zero_()
        before = batch(), viewed()
        refused(LP_ERR_STATE, e.focus_create, slots=3)   # no tracker
        refused(LP_ERR_STATE, run_focus, e, dev, None)
        e.tracker_create(n_streams=2, max_tracks=16)
        refused(LP_ERR_STATE, run_focus, e, dev, None)   # a tracker, no plan
        refused(LP_ERR_STATE, e.focus_plan, [H], [W])
        refused(LP_ERR_STATE, e.focus_state, 0)
        refused(LP_ERR_ARG, e.focus_create, slots=17)
        e.focus_create(slots=3, **FCFG)
        dev.dd.zero_()
        assert (batch(), viewed()) == before, "a focus plan that was never used changed another entry point's output"
        seed(e, 0, TRACKS_A)
        good = run_focus(e, dev, [0, 1])
        e.focus_create(slots=3, **FCFG)   # again: the cursors restart, so the call below repeats `good`
        assert e.focus_state(0) == {"cursor": 0, "unserved": 0}
        small = torch.zeros(2 * 8 * 800 * 3, dtype=torch.uint8, device="cuda")
        bad = {"B x (1 + slots) > max_batch": lambda: e.run_focus_device(dev.img.data_ptr(), 3, H, W, CONF, IOU, MIN_AREA, dev.dd.data_ptr(),
                                                                          dev.dc.data_ptr(), stream_ids=[0, 1, 0]),
               "a stream id out of range": lambda: run_focus(e, dev, [0, 2]),
               "a negative stream id": lambda: run_focus(e, dev, [-1, 0]),
               "a frame below 16 pixels": lambda: e.run_focus_device(small.data_ptr(), 2, 8, 800, CONF, IOU, MIN_AREA, dev.dd.data_ptr(),
                                                                     dev.dc.data_ptr()),
               "plan: a frame below 16 pixels": lambda: e.focus_plan([H, 15], [W, W]),
               "plan: a stream id out of range": lambda: e.focus_plan([H], [W], [5]),
               "host: a frame below 16 pixels": lambda: e.run_focus([f0, np.ascontiguousarray(f1[:10])], CONF, IOU, MIN_AREA),
               "host: too many frames": lambda: e.run_focus([f0, f1, f0], CONF, IOU, MIN_AREA)}
        for what, fn in bad.items():
            refused(LP_ERR_ARG, fn)
            assert e.focus_state(0) == {"cursor": 0, "unserved": 0}, f"{what}: the refused call moved the plan's state"
        again = run_focus(e, dev, [0, 1])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(good, again)), "the handle gives another result after the refused calls"
        dev.dd.zero_()
        assert (batch(), viewed()) == before
        e.tracker_create(n_streams=1)   # replaces the tracker: the plan goes with it
        refused(LP_ERR_STATE, run_focus, e, dev, None)
        e.focus_create(slots=3)
        e.tracker_reset(-1)
        e.focus_plan([H], [W])
        assert e.focus_state(0)["cursor"] == 3, "lp_tracker_reset touched the plan"
        e.focus_destroy()
        refused(LP_ERR_STATE, e.focus_state, 0)
    finally:
        e.close()


def _sequence(models, n=6):
    """a patch moving 4 pixels a frame over frame 0"""
    rng = np.random.default_rng(3)
    patch = rng.integers(0, 256, (48, 48, 3), dtype=np.uint8)
    seq = []
    for k in range(n):
        f = models["frames"][1].copy()
        f[300:348, 400 + 4 * k:448 + 4 * k] = patch
        seq.append(f)
    return seq


def test_tracker_and_inventory_behind_run_focus_device(models):
    from litepi._ffi import TRACK_DTYPE
    seq = _sequence(models)
    e = _engine(models, "fp16", 4, classifier=False)
    try:
        e.load_classifier(models["sd"])
        e.tracker_create(n_streams=1, max_tracks=256, max_age=1, min_hits=2)
        e.inventory_create()
        e.focus_create(slots=3, **FCFG)
        dev = Dev(e, [seq[0]], 3)
        dt = torch.zeros(e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        placed, tracked = 0, 0   # placed: reported only, the seeded detector's boxes need not be small
        for k, f in enumerate(seq):
            dev.img.copy_(torch.from_numpy(f[None]))
            torch.cuda.synchronize()
            e.run_focus_device(dev.img.data_ptr(), 1, H, W, CONF, IOU, MIN_AREA, dev.dd.data_ptr(), dev.dc.data_ptr(), dev_views=dev.dv.data_ptr())
            e.track_device(dev.dd.data_ptr(), dev.dc.data_ptr(), 1, dt.data_ptr())
            e.inventory_device(dev.dd.data_ptr(), dev.dc.data_ptr(), dt.data_ptr(), 1, crops=True)
            recs, cnt, views = dev.result(e)
            n = int(cnt[0])
            assert n >= 1, f"frame {k} keeps no detection"
            tr = dt.cpu().numpy().view(TRACK_DTYPE)[:n]
            tracked += int((tr["hits"] >= 2).sum())
            assert len(windows(views[0])) == 3
            if k > 0:   # small tracks exist from the second frame on: the first window is theirs, not the sweep's
                placed += windows(views[0])[0] not in R.view_grid(320, 64, H, W)
        assert tracked >= 1, "nothing was tracked over two frames"
        print(f"{placed} of {len(seq) - 1} frames placed a window for a track")
        e.inventory_flush(-1)
        signs, crops, _ = e.inventory_drain(crops=True)
        assert len(signs) >= 1 and (signs["flags"] & 1).any(), "no sign with a crop came out"
    finally:
        e.close()


def test_pipeline_and_cli_report_their_windows(models, tmp_path, capsys):
    from litepi import HybridPipeline, e2e
    seq = _sequence(models)
    tcfg = dict(n_streams=1, max_tracks=256, max_age=1, min_hits=2)
    kw = dict(num_classes=91, det_input_size=S, precision="fp16", max_det=300)
    for bad in (dict(focus=2), dict(focus=2, track=True, views=["full"]), dict(focus=2, track=True, tile_overlap=64),
                dict(focus=2, track=True, view_tile=480), dict(focus=4, track=True, max_batch=4), dict(focus_config=dict(margin=3.0), track=True)):
        with pytest.raises(ValueError):
            HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", **dict(kw, max_batch=bad.pop("max_batch", 6)), **bad)
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", max_batch=6, track=True, track_config=tcfg, focus=2,
                          focus_config=FCFG, **kw)
    e = _engine(models, "fp16", 6, classifier=False)
    try:
        e.load_classifier(models["sd"])
        e.tracker_create(**tcfg)
        e.focus_create(slots=2, **FCFG)
        seen = []
        for k in range(0, 6, 2):   # two frames of one stream per run_batch: two engine calls, the tracker fed between them
            outs = pipe.run_batch(seq[k:k + 2], CONF, IOU, MIN_AREA)
            assert np.asarray(pipe.last_focus_views).shape == (2, 2, 4)
            for i, (res, _) in enumerate(outs):
                d, c, _, _, views = e.run_focus([seq[k + i]], CONF, IOU, MIN_AREA)
                tr = e.track(d, np.asarray(c, dtype=np.int32))
                n = int(c[0])
                assert n >= 1 and len(res) == n, f"frame {k + i}"
                assert pipe.last_focus_views[i] == views[0].tolist(), f"frame {k + i}: the pipeline used other windows"
                assert [(r["det_conf"], r["track_id"], r["track_hits"]) for r in res] == \
                       [(float(x["det_conf"]), int(t["track_id"]), int(t["hits"])) for x, t in zip(d[0, :n], tr[0, :n])], f"frame {k + i}"
                seen.append(views[0].tolist())
        assert len({json.dumps(v) for v in seen}) >= 3, "the windows never changed"
    finally:
        pipe.close()
        e.close()
    np.stack(seq).tofile(tmp_path / "clip.bgr")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(91)}))
    out = tmp_path / "out"
    common = ["--detector_param", models["param"], "--detector_bin", models["bin"], "--classifier", models["cls"], "--clf_arch", "shufflenetv2",
            "--labels", str(tmp_path), "--classes", str(classes), "--batch_images", "2", "--max_det", "300", "--det_input_size", str(S),
            "--raw_frames", str(tmp_path / "clip.bgr"), "--frame_size", f"{W}x{H}", "--output", str(out), "--track_max_age", "1",
              "--track_min_hits", "2", "--benchmark_conf", str(CONF), "--yolo_conf", str(CONF)]
    argv = common + ["--track", "--focus", "2", "--focus_margin", "2.5"]
    assert e2e.main(argv) == 0
    assert "Focus views:" in capsys.readouterr().out
    with open(out / "m+shufflenetv2" / "focus.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["frame", "slot", "x", "y", "w", "h"] and len(rows) == 1 + 6 * 2
    assert [r[:2] for r in rows[1:5]] == [["0", "0"], ["0", "1"], ["1", "0"], ["1", "1"]]
    assert all(int(r[4]) >= 16 and int(r[5]) >= 16 for r in rows[1:]), "an empty slot under a sweep"
    for bad in (["--focus", "2"], ["--track", "--focus", "2", "--views", "full"], ["--track", "--focus", "17"]):
        with pytest.raises(SystemExit):
            e2e.main(common + bad)
