"""GPU tests of the evidence store (include/litepi.h, lp_evidence_*): the device store against the NumPy restatement of the rule
(tests/evidence_ref.py), byte for byte.  Tests 1-5 are model-free: frames through lp_test_set_frames, ROI lists through
lp_test_set_rois, records through lp_inventory.

1. windows: boxes in the middle, on every edge and corner, wider than the frame, 2-pixel, empty and NaN; two frame sizes, two E;
2. ordering within one call: a best improved three times, a track that opens, peaks and closes inside the call, a best that
   predates the call, a slot reused after a close, a flush; the same records in calls of 1, 2 and 5 frames;
3. three streams interleaved in one call == each stream alone;  4. a full log;
5. a crops = 0 call between two crops = 1 calls; the old drain on a handle with a store; 5b. windows whose rows exceed the
   staged LDS rows (720 x 1280 frames: the per-pixel form); a call of another kind forgets the frames;
6. a store changes no sign, crop, tracker output or launch list;  7. behind the pipeline: BGR, NV12, views;  8. errors;
9. HybridPipeline(evidence=...) and e2e --inventory_evidence."""
import numpy as np
import pytest
import torch

import evidence_ref as E
import inventory_ref as V
import pixfmt_ref as P
import tracking_ref as R

pytestmark = pytest.mark.gpu

NC = 58
S = 64
MD = 8
F = np.float32


# ---------------------------------------------------------------------------- helpers
@pytest.fixture(scope="module")
def eng():
    """a handle without models: the store needs none"""
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=16, max_det=MD, num_classes=NC)
    yield e
    e.close()


def frames_of(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def records(frames):
    """frames: a list of [(slot, track_id, (x1, y1, x2, y2))] -> dets, tracks [B, MD], counts [B]"""
    dets, trk = np.zeros((len(frames), MD), dtype=R.DET_DTYPE), np.zeros((len(frames), MD), dtype=R.TRACK_DTYPE)
    counts = np.zeros(len(frames), np.int32)
    for b, recs in enumerate(frames):
        counts[b] = len(recs)
        for i, (slot, tid, box) in enumerate(recs):
            dets[b, i]["x1"], dets[b, i]["y1"], dets[b, i]["x2"], dets[b, i]["y2"] = box
            dets[b, i]["det_conf"], dets[b, i]["cls_class"] = 0.5, -1
            trk[b, i]["track_id"], trk[b, i]["slot"], trk[b, i]["hits"] = tid, slot, 3
    return dets, trk, counts


def feed(eng, ref, d, t, c, frames, sid=None, crops=True, call=0):
    """one lp_inventory call on both sides; crops: every record has a classifier crop whose bytes name it"""
    B = len(c)
    if crops:
        recs = [(b, i) for b in range(B) for i in range(min(max(int(c[b]), 0), MD))]
        pix = np.zeros((len(recs), S, S, 3), np.uint8)
        for j, (b, i) in enumerate(recs):
            pix[j] = (7 * call + 31 * b + 3 * i) % 256
        eng.test_set_frames(frames)
        eng.test_set_rois(pix, [b for b, _ in recs], [i for _, i in recs])
        eng.inventory(d, c, t, sid, crops=True)
        ref.feed(d, t, c, sid, crops={r: pix[j] for j, r in enumerate(recs)}, frames=frames)
    else:
        eng.inventory(d, c, t, sid, crops=False)
        ref.feed(d, t, c, sid, frames=None)


def assert_signs_equal(got, want, tag):
    assert len(got) == len(want), f"{tag}: {len(got)} signs, want {len(want)}"
    for name in got.dtype.names:
        bad = got[name].view(np.int32) != want[name].view(np.int32)
        if got[name].dtype.kind == "f":   # bit-equal, but a NaN equals any NaN: its sign and payload are nobody's rule
            bad &= ~(np.isnan(got[name]) & np.isnan(want[name]))
        bad = np.flatnonzero(bad)
        assert len(bad) == 0, f"{tag}: field {name}, sign {bad[0]}: got {got[name][bad[0]]!r}, want {want[name][bad[0]]!r}"


def assert_pictures_equal(gp, gw, wp, ww, tag):
    assert gw.tolist() == ww.tolist(), f"{tag}: windows {gw.tolist()}, want {ww.tolist()}"
    assert gp.shape == wp.shape
    for k in range(len(gp)):
        bad = np.argwhere(gp[k] != wp[k])
        assert len(bad) == 0, f"{tag}: picture {k} (window {gw[k].tolist()}) differs in {len(bad)} bytes, first at {bad[0].tolist()}"


def assert_drain_equal(eng, ref, tag, by_stream=False):
    gs, gc, gp, gw, gd = eng.inventory_drain_evidence()
    ws, wc, wp, ww, wd = ref.drain_evidence()
    if by_stream:   # across the streams of a call the order of blocks is unspecified
        go, wo = np.argsort(gs["stream"], kind="stable"), np.argsort(ws["stream"], kind="stable")
        gs, gc, gp, gw, ws, wc, wp, ww = gs[go], gc[go], gp[go], gw[go], ws[wo], wc[wo], wp[wo], ww[wo]
    assert_signs_equal(gs, ws, tag)
    assert gd == wd, f"{tag}: dropped {gd}, want {wd}"
    assert gc.tobytes() == wc.tobytes(), f"{tag}: crops differ"
    assert_pictures_equal(gp, gw, wp, ww, tag)
    return gs, gp, gw


def assert_open_equal(eng, ref, stream, tag):
    assert_signs_equal(eng.inventory_open(stream), ref.open(stream), tag + " open")
    gp, gw = eng.evidence_open(stream)
    wp, ww = ref.open_evidence(stream)
    assert_pictures_equal(gp, gw, wp, ww, tag + " open")


def create(eng, tcfg, icfg, ecfg):
    eng.tracker_create(**tcfg)
    eng.inventory_create(**icfg)
    eng.evidence_create(**ecfg)
    return E.EvidenceRef(MD, tcfg, icfg, ev_cfg=ecfg)


# ---------------------------------------------------------------------------- 1. windows
@pytest.mark.parametrize("H, W", [(48, 80), (97, 131)])
@pytest.mark.parametrize("size", [32, 64])
def test_windows(eng, H, W, size):
    boxes = [(W / 2 - 6, H / 2 - 5, W / 2 + 6, H / 2 + 5),                                    # the middle
             (0, H / 2 - 4, 9, H / 2 + 4), (W - 9, H / 2 - 4, W, H / 2 + 4), (W / 2 - 5, 0, W / 2 + 5, 8), (W / 2 - 5, H - 8, W / 2 + 5, H),
             (0, 0, 10, 10), (W - 10, 0, W, 10), (0, H - 10, 10, H), (W - 10.5, H - 10.5, W, H),
             (2, 3, 2 + 0.75 * W, 3 + 0.3 * H),                                                # side > W: a non-square window, bars
             (20.25, 11.5, 22.25, 13.5),                                                      # a 2-pixel box: side 16
             (-20, -20, W + 20, H + 20),                                                      # larger than the frame: the whole frame
             (30, 30, 30, 40), (40, 30, 30, 40), (np.nan, 3, 9, 9)]                           # no picture
    ref = create(eng, dict(max_tracks=8, max_age=50, min_hits=1), {}, dict(size=size, scale=2.0))
    fr = frames_of(2, H, W, H + size)
    d, t, c = records([[(s, 1 + s, b) for s, b in enumerate(boxes[:8])], [(s, 11 + s, b) for s, b in enumerate(boxes[8:])]])
    feed(eng, ref, d, t, c, fr)
    tag = f"{W}x{H} E {size}"
    assert_open_equal(eng, ref, 0, tag)
    op = eng.inventory_open(0)
    assert (op["flags"] & E.HAS_EVIDENCE != 0).tolist() == [True] * 4 + [False] * 3 + [True]
    wins = eng.evidence_open(0)[1]
    assert wins[1].tolist()[2] == W and wins[3].tolist()[2:] == [W, H]   # slots 1 (wide box) and 3 (larger than the frame)
    assert wins[2].tolist()[2:] == [16, 16]
    eng.inventory_flush()
    ref.flush()
    signs, pics, _ = assert_drain_equal(eng, ref, tag)
    assert len(signs) == 15 and (signs["flags"] & E.HAS_EVIDENCE != 0).sum() == 12
    assert (pics[(signs["flags"] & E.HAS_EVIDENCE) == 0] == 0).all()


# ---------------------------------------------------------------------------- 2. ordering within one call
def ordering_scene():
    """12 frames of one stream, max_age = 1 (slot, id, box); entry (0, 1) is opened by a call of its own before"""
    sq = lambda x, y, s: (x, y, x + s, y + s)   # noqa: E731
    fr = [[] for _ in range(12)]
    for f, s in enumerate((5, 4)):                 # A (slot 0, id 1): its best predates the call; closes at frame 3
        fr[f].append((0, 1, sq(8, 8, s)))
    for f in range(5, 12):                         # slot 0 reused after the close, stays open
        fr[f].append((0, 10, sq(50, 20, 6 + (f == 7) * 5)))
    for f, s in enumerate((4, 6, 5, 8, 7, 10, 9, 9, 3, 3, 3, 3)):   # B (slot 1, id 2): improves three times, stays open
        fr[f].append((1, 2, sq(30 + f, 10, s)))
    for f, s in ((2, 5), (3, 7), (4, 11), (5, 6)):   # C (slot 2, id 3): opens, peaks and closes (frame 7) inside the call
        fr[f].append((2, 3, sq(60, 30 - f, s)))
    for f in (6, 7):                               # D (slot 3, id 4), closed at frame 8 by another id in its slot
        fr[f].append((3, 4, sq(12, 28, 9 - f + 6)))
    for f in range(8, 12):
        fr[f].append((3, 5, sq(14, 26, 5 + f % 2)))
    return records([[(0, 1, sq(6, 6, 9))]]), records(fr)


@pytest.mark.parametrize("split", [12, 1, 2, 5])
def test_ordering_within_one_call(eng, split):
    (d0, t0, c0), (d, t, c) = ordering_scene()
    H, W = 48, 80
    fr0, fr = frames_of(1, H, W, 5), frames_of(12, H, W, 6)
    ref = create(eng, dict(max_tracks=8, max_age=1, min_hits=1), {}, dict(size=32, scale=2.5))
    feed(eng, ref, d0, t0, c0, fr0)
    for k, i in enumerate(range(0, 12, split)):
        feed(eng, ref, d[i:i + split], t[i:i + split], c[i:i + split], fr[i:i + split], call=k + 1)
    tag = f"split {split}"
    assert_open_equal(eng, ref, 0, tag)
    assert eng.inventory_open(0)["track_id"].tolist() == [10, 2, 5]
    eng.inventory_flush()
    ref.flush()
    signs, pics, wins = assert_drain_equal(eng, ref, tag)
    assert signs["track_id"].tolist() == [1, 3, 4, 10, 2, 5] and (signs["flags"] & E.HAS_EVIDENCE).all()
    # spelled out from the records: A keeps the picture of the call before, B's is its fourth best, C's its peak
    want = {1: (fr0[0], (6, 6, 15, 15)), 2: (fr[5], (35, 10, 45, 20)), 3: (fr[4], (60, 26, 71, 37)), 10: (fr[7], (50, 20, 61, 31))}
    for k, tid in enumerate(signs["track_id"].tolist()):
        if tid in want:
            frame, box = want[tid]
            win = E.window(F(2.5), H, W, box)[0]
            assert wins[k].tolist() == list(win) and pics[k].tobytes() == E.picture(frame, 32, win).tobytes(), f"{tag}: track {tid}"


# ---------------------------------------------------------------------------- 3. streams
def test_three_streams_interleaved_equal_each_alone(eng):
    H, W = 131, 173   # (make_scene keeps its signs 60 pixels off the borders at birth)
    tcfg, ecfg = dict(n_streams=3, max_tracks=8, max_age=1, min_hits=1), dict(size=32, scale=2.0)
    scenes = [R.make_scene(900 + s, max_det=MD, num_classes=NC, n_frames=8, n_signs=5, frame_hw=(H, W)) for s in range(3)]
    frames = [frames_of(8, H, W, 40 + s) for s in range(3)]
    # the tracks of every stream from a tracker of its own
    eng.tracker_create(**tcfg)
    tracks = [eng.track(scenes[s][0], scenes[s][1], [s] * 8) for s in range(3)]
    alone = []
    for s in range(3):
        ref = create(eng, tcfg, {}, ecfg)
        for i in (0, 4):
            feed(eng, ref, scenes[s][0][i:i + 4], tracks[s][i:i + 4], scenes[s][1][i:i + 4], frames[s][i:i + 4], [s] * 4)
        eng.inventory_flush()
        ref.flush()
        alone.append(assert_drain_equal(eng, ref, f"stream {s} alone"))
    ref = create(eng, tcfg, {}, ecfg)
    for i in (0, 4):   # 12 frames per call: s0 f0, s1 f0, s2 f0, s0 f1, ...
        order = [(s, f) for f in range(i, i + 4) for s in range(3)]
        pick = lambda a: np.stack([a[s][f] for s, f in order])   # noqa: E731
        feed(eng, ref, pick([sc[0] for sc in scenes]), pick(tracks), np.array([scenes[s][1][f] for s, f in order], np.int32),
             pick(frames), [s for s, _ in order])
    for s in range(3):
        assert_open_equal(eng, ref, s, f"interleaved, stream {s}")
    eng.inventory_flush()
    ref.flush()
    signs, pics, wins = assert_drain_equal(eng, ref, "interleaved", by_stream=True)
    assert len(signs) >= 3 and (signs["flags"] & E.HAS_EVIDENCE).any()
    for s in range(3):
        m = signs["stream"] == s
        assert_signs_equal(signs[m], alone[s][0], f"stream {s} of the interleaved call")
        assert_pictures_equal(pics[m], wins[m], alone[s][1], alone[s][2], f"stream {s} of the interleaved call")


# ---------------------------------------------------------------------------- 4. a full log
def test_log_full(eng):
    H, W = 131, 173
    tcfg = dict(max_tracks=8, max_age=0, min_hits=1)
    dets, counts = R.make_scene(321, max_det=MD, num_classes=NC, n_frames=16, n_signs=9, frame_hw=(H, W))
    fr = frames_of(16, H, W, 9)
    eng.tracker_create(**tcfg)
    tracks = eng.track(dets, counts)
    ref = create(eng, tcfg, dict(max_signs=3), dict(size=32, scale=2.0))
    feed(eng, ref, dets, tracks, counts, fr)
    eng.inventory_flush()
    ref.flush()
    assert ref.dropped >= 2 and len(ref.log) == 3
    assert_drain_equal(eng, ref, "full log")
    feed(eng, ref, dets[:6], tracks[:6], counts[:6], fr[:6], call=1)   # a drain re-arms it
    eng.inventory_flush()
    ref.flush()
    signs, _, _ = assert_drain_equal(eng, ref, "after the drain")
    assert len(signs) >= 1


# ---------------------------------------------------------------------------- 5. crops = 0 between crops = 1; the old drain
def test_crops_0_call_between_and_the_old_drain(eng):
    H, W = 48, 80
    sq = lambda x, y, s: (x, y, x + s, y + s)   # noqa: E731
    ref = create(eng, dict(max_tracks=8, max_age=3, min_hits=1), {}, dict(size=32, scale=2.0))
    fr = frames_of(3, H, W, 12)
    calls = [records([[(0, 1, sq(10, 10, 5)), (1, 2, sq(40, 10, 9)), (2, 3, sq(60, 30, 4))]]),
             records([[(0, 1, sq(10, 10, 7)), (1, 2, sq(40, 10, 8)), (2, 3, sq(60, 30, 6))]]),   # 1 and 3 improve without frames
             records([[(0, 1, sq(10, 10, 6)), (1, 2, sq(40, 10, 7)), (2, 3, sq(60, 30, 8))]])]   # 3 improves again, with frames
    for k, (d, t, c) in enumerate(calls):
        feed(eng, ref, d, t, c, fr[k:k + 1], crops=k != 1, call=k)
        assert_open_equal(eng, ref, 0, f"call {k}")
    assert (eng.inventory_open(0)["flags"] & E.HAS_EVIDENCE).tolist() == [0, 4, 4]
    eng.inventory_flush()
    ref.flush()
    gs, gc, gd = eng.inventory_drain()   # the old drain: the signs and crops, the pictures are discarded
    ws, wc, wd = ref.drain()
    assert_signs_equal(gs, ws, "old drain")
    assert gc.tobytes() == wc.tobytes() and gd == wd and len(gs) == 3
    assert len(eng.inventory_drain_evidence()[0]) == 0


# ---------------------------------------------------------------------------- 5b. windows beyond the staged rows
def test_wide_windows_take_the_per_pixel_form(eng):
    """a 720 x 1280 frame: window rows longer than the kernel's 2 KB staged rows (windows beyond 672 pixels), as an HD video
    gives for any sign beyond ~336 pixels at scale 2, next to a small window in the same launch: frame -> log for an entry
    that closes within the call, frame -> gallery for entries that stay open, gallery -> log in the call after"""
    H, W = 720, 1280
    ref = create(eng, dict(max_tracks=8, max_age=0, min_hits=1), {}, dict(size=64, scale=2.0))
    fr = frames_of(3, H, W, 77)
    d, t, c = records([[(0, 1, (100, 100, 440, 300)),       # side 680: closes in frame 1 with this best
                        (1, 2, (-50, 200, 1400, 500)),      # wider than the frame: the whole frame, stays the best
                        (2, 3, (600, 600, 640, 650))],      # a staged window
                       [(0, 4, (500.5, 50, 900.5, 400)),    # 800 x 720, stays open
                        (1, 2, (0, 300, 700, 450)),
                        (2, 3, (600, 600, 700, 700))]])
    feed(eng, ref, d, t, c, fr[:2])
    assert_open_equal(eng, ref, 0, "wide, open")
    wins = eng.evidence_open(0)[1].tolist()
    assert [w[2:] for w in wins] == [[800, 720], [1280, 720], [200, 200]]
    signs, _, wl = assert_drain_equal(eng, ref, "wide, closed within the call")
    assert signs["track_id"].tolist() == [1] and wl[0].tolist()[2:] == [680, 680]
    d, t, c = records([[(1, 9, (300, 300, 1100, 700))]])   # everything closes: three gallery -> log copies; 9 opens on 1280 x 720
    feed(eng, ref, d, t, c, fr[2:], call=1)
    assert_open_equal(eng, ref, 0, "wide, reused slot")
    signs, _, _ = assert_drain_equal(eng, ref, "wide, gallery -> log")
    assert signs["track_id"].tolist() == [4, 2, 3] and (signs["flags"] & E.HAS_EVIDENCE).all()


# ---------------------------------------------------------------------------- models for 6 and 7
CONF, IOU, MIN_AREA = 0.05, 0.45, 50
PH, PW = 240, 320


@pytest.fixture(scope="module")
def cls_state():
    from litepi.backend import random_shufflenet_state
    return random_shufflenet_state(91, seed=3)


def model_engine(synth_models, cls_state, max_det=32):
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=8, max_det=max_det, num_classes=91)
    e.load_detector(*synth_models["v1"])
    e.load_classifier(cls_state)
    return e


def clip(seed, n_calls=3, B=2):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (B, PH, PW, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    out = []
    for k in range(n_calls):
        f = base.copy()
        f[:, 100:140, 80 + 4 * k:120 + 4 * k] = patch
        out.append(f)
    return out


# ---------------------------------------------------------------------------- 6. no effect without a store
def test_store_changes_nothing_else(synth_models, cls_state):
    from litepi._ffi import TRACK_DTYPE
    dev = torch.device("cuda", 0)
    calls = clip(5)
    B = 2
    sid = np.arange(B, dtype=np.int32)
    results = []
    for with_store in (False, True):
        e = model_engine(synth_models, cls_state)
        try:
            e.tracker_create(n_streams=B, max_tracks=64, max_age=0, min_hits=1, iou_match=0.5)
            e.inventory_create()
            if with_store:
                e.evidence_create(size=64)
            d = torch.zeros(B * 32 * 32, dtype=torch.uint8, device=dev)
            c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
            t = torch.zeros(B * 32 * 32, dtype=torch.uint8, device=dev)
            trk = []
            for k, frames in enumerate(calls + calls[:1]):
                x = torch.from_numpy(frames).to(dev)
                if k == len(calls):
                    e.profile_next(True)
                e.run_batch_device(x.data_ptr(), B, PH, PW, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
                e.track_device(d.data_ptr(), c.data_ptr(), B, t.data_ptr(), sid)
                e.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=True)
                e.synchronize()
                trk.append(t.cpu().numpy().view(TRACK_DTYPE).tobytes())
            launches = [(r["name"], r["layer"]) for r in e.profile_read()]
            e.inventory_flush()
            signs, crops, _ = e.inventory_drain()
            snap = e.tracker_snapshot(0)
            results.append((signs, crops, trk, launches, snap["tracks"].tobytes(), snap["next_id"]))
        finally:
            e.close()
    a, b = results
    assert len(a[0]) >= 1 and (b[0]["flags"] & E.HAS_EVIDENCE).any() and not (a[0]["flags"] & E.HAS_EVIDENCE).any()
    oa, ob = np.argsort(a[0]["stream"], kind="stable"), np.argsort(b[0]["stream"], kind="stable")
    sb = b[0][ob].copy()
    sb["flags"] &= ~E.HAS_EVIDENCE
    assert_signs_equal(sb, a[0][oa], "signs apart from LP_SIGN_HAS_EVIDENCE")
    assert a[1][oa].tobytes() == b[1][ob].tobytes(), "crops differ on a handle that has a store"
    assert a[2] == b[2] and a[4:] == b[4:], "the tracker's output differs on a handle that has a store"
    assert a[3] == b[3] and len(a[3]) > 10, "the pipeline's launch list differs on a handle that has a store"
    assert not any("evidence" in name or "inventory" in name for name, _ in a[3])


def test_another_call_on_the_handle_forgets_the_frames(synth_models, cls_state):
    """lp_classify rewrites the handle's source buffer and geometry table: a crops = 1 call behind it is refused, not served
    from what the pipeline call before left there"""
    from litepi import _ffi
    dev = torch.device("cuda", 0)
    frames = clip(5)[0]
    B = 2
    e = model_engine(synth_models, cls_state)
    try:
        e.tracker_create(n_streams=B, max_tracks=64, max_age=0, min_hits=1, iou_match=0.5)
        e.inventory_create()
        e.evidence_create(size=32)
        d = torch.zeros(B * 32 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        t = torch.zeros(B * 32 * 32, dtype=torch.uint8, device=dev)
        x = torch.from_numpy(frames).to(dev)
        sid = np.arange(B, dtype=np.int32)
        e.run_batch_device(x.data_ptr(), B, PH, PW, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
        e.track_device(d.data_ptr(), c.data_ptr(), B, t.data_ptr(), sid)
        e.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=True)
        e.synchronize()
        before = e.inventory_open(0)
        e.classify([np.full((20, 30, 3), 90, np.uint8)])
        with pytest.raises(_ffi.LitepiError) as ei:
            e.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=True)
        assert ei.value.code == _ffi.LP_ERR_STATE
        assert_signs_equal(e.inventory_open(0), before, "after the refused call")
        e.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=False)   # crops = 0 needs no frames
        e.run_batch_device(x.data_ptr(), B, PH, PW, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
        e.track_device(d.data_ptr(), c.data_ptr(), B, t.data_ptr(), sid)
        e.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=True)
        e.synchronize()
    finally:
        e.close()


# ---------------------------------------------------------------------------- 7. behind the pipeline
@pytest.mark.parametrize("mode", ["bgr", "nv12", "views"])
def test_evidence_behind_the_pipeline(synth_models, cls_state, mode):
    dev = torch.device("cuda", 0)
    calls = clip(11, n_calls=4)
    B, size, scale = 2, 64, 2.0
    sid = np.arange(B, dtype=np.int32)
    shown = calls
    if mode == "nv12":
        nv = [np.stack([P.bgr_to_nv12(f) for f in call]) for call in calls]
        shown = [np.stack([P.nv12_to_bgr(f, "bt601") for f in call]) for call in nv]   # the frames the handle holds
    e = model_engine(synth_models, cls_state)
    try:
        if mode == "nv12":
            e.set_input_format("nv12", "bt601")
        e.tracker_create(n_streams=B, max_tracks=64, max_age=0, min_hits=1, iou_match=0.5)
        e.inventory_create()
        e.evidence_create(size=size, scale=scale)
        d = torch.zeros(B * 32 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        t = torch.zeros(B * 32 * 32, dtype=torch.uint8, device=dev)
        src = [np.ascontiguousarray(nv[k] if mode == "nv12" else calls[k]) for k in range(len(calls))]
        x = torch.zeros(src[0].shape, dtype=torch.uint8, device=dev)   # one buffer: the step's key holds its address
        for k in range(len(calls)):
            e.synchronize()   # the frames stay unwritten until the stream has passed the inventory call
            x.copy_(torch.from_numpy(src[k]))
            torch.cuda.synchronize()
            if mode == "views":
                e.run_views_device(x.data_ptr(), B, PH, PW, ["full", (40, 30, 200, 160)], CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
            else:
                e.run_batch_device(x.data_ptr(), B, PH, PW, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
            e.track_device(d.data_ptr(), c.data_ptr(), B, t.data_ptr(), sid)
            e.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=True)
        stats = e.graph_stats()
        assert stats["replays"] >= len(calls) - 2, f"{mode}: the step no longer replays: {stats}"
        e.inventory_flush()
        signs, _, pics, wins, dropped = e.inventory_drain_evidence()
        assert dropped == 0 and len(signs) >= 2 and (signs["flags"] & E.HAS_EVIDENCE).sum() >= 2, f"{mode}: {len(signs)} signs"
        for k, s in enumerate(signs):
            frame = shown[int(s["best_frame"])][int(s["stream"])]
            win, has = E.window(F(scale), PH, PW, (s["x1"], s["y1"], s["x2"], s["y2"]))
            assert has == bool(s["flags"] & E.HAS_EVIDENCE) and wins[k].tolist() == list(win), f"{mode}: sign {k}"
            want = E.picture(frame, size, win) if has else np.zeros((size, size, 3), np.uint8)
            bad = np.argwhere(pics[k] != want)
            assert len(bad) == 0, f"{mode}: sign {k} (track {s['track_id']}, frame {s['best_frame']}, window {win}): {len(bad)} bytes differ"
    finally:
        e.close()


# ---------------------------------------------------------------------------- 8. errors
def test_errors_leave_the_handle_usable():
    from litepi import Engine, _ffi
    from litepi._ffi import LitepiError
    e = Engine(precision="fp16", max_batch=4, max_det=MD, num_classes=NC)

    def code(fn):
        with pytest.raises(LitepiError) as ei:
            fn()
        return ei.value.code
    try:
        fr = frames_of(1, 48, 80, 3)
        d, t, c = records([[(0, 1, (10, 10, 20, 20))]])
        e.tracker_create(max_tracks=8, max_age=1, min_hits=1)
        assert code(lambda: e.evidence_create()) == _ffi.LP_ERR_STATE          # no inventory
        e.inventory_create(keep_crops=0)
        assert code(lambda: e.evidence_create()) == _ffi.LP_ERR_ARG            # keep_crops = 0
        e.inventory_create()
        for kw in (dict(size=40), dict(size=16), dict(size=512), dict(scale=0.5), dict(scale=float("nan"))):
            assert code(lambda: e.evidence_create(**kw)) == _ffi.LP_ERR_ARG, kw
        import ctypes as C
        n = C.c_int()
        assert e.lib.lp_inventory_drain_evidence(e._h, None, None, None, None, 0, C.byref(n), None) == _ffi.LP_ERR_STATE   # no store
        assert e.lib.lp_evidence_open(e._h, 0, None, None, 0, C.byref(n)) == _ffi.LP_ERR_STATE
        e.evidence_destroy()   # without one: fine
        e.evidence_create(size=32)
        assert code(lambda: e.inventory(d, c, t, crops=True)) == _ffi.LP_ERR_STATE   # the handle remembers no frames
        assert code(lambda: e.test_set_frames(np.zeros((5, 48, 80, 3), np.uint8))) == _ffi.LP_ERR_ARG   # more than max_batch
        assert code(lambda: e.evidence_open(1)) == _ffi.LP_ERR_ARG
        assert len(e.inventory_open(0)) == 0   # refused before anything was enqueued
        ref = E.EvidenceRef(MD, dict(max_tracks=8, max_age=1, min_hits=1), ev_cfg=dict(size=32))
        feed(e, ref, d, t, c, fr)
        assert_open_equal(e, ref, 0, "after the refused calls")
        e.evidence_create(size=64)   # replaced: the open entry keeps its record and loses its picture
        assert e.inventory_open(0)["flags"].tolist() == [V.HAS_CROP]
        e.inventory_flush()
        signs, _, pics, wins, _ = e.inventory_drain_evidence()
        assert len(signs) == 1 and pics.shape == (1, 64, 64, 3) and not pics.any() and not wins.any()
        out = np.zeros(4, dtype=_ffi.SIGN_DTYPE)
        ref = E.EvidenceRef(MD, dict(max_tracks=8, max_age=1, min_hits=1), ev_cfg=dict(size=64))
        ref.frame_no[0] = 1
        d2, t2, c2 = records([[(0, 1, (10, 10, 20, 20)), (1, 2, (30, 5, 50, 30))]])
        feed(e, ref, d2, t2, c2, fr)
        e.inventory_flush()
        ref.flush()
        assert e.lib.lp_inventory_drain_evidence(e._h, out.ctypes.data, None, None, None, 1, C.byref(n), None) == _ffi.LP_ERR_ARG   # short cap
        assert_drain_equal(e, ref, "after the refused drain")
        # the store goes with its inventory and with its tracker
        e.inventory_create()
        assert not hasattr(e, "ev_cfg") and e.lib.lp_evidence_open(e._h, 0, None, None, 0, C.byref(n)) == _ffi.LP_ERR_STATE
        e.evidence_create()
        e.inventory_destroy()
        assert code(lambda: e.evidence_create()) == _ffi.LP_ERR_STATE
        e.inventory_create()
        e.evidence_create()
        e.tracker_create(max_tracks=8)
        assert code(lambda: e.evidence_create()) == _ffi.LP_ERR_STATE
        e.inventory_create()
        e.evidence_create(size=32)
        e.tracker_destroy()
        e.evidence_destroy()   # without a tracker: fine
        e.tracker_create(max_tracks=8, max_age=1, min_hits=1)
        e.inventory_create()
        e.evidence_create(size=32)
        ref = E.EvidenceRef(MD, dict(max_tracks=8, max_age=1, min_hits=1), ev_cfg=dict(size=32))
        feed(e, ref, d, t, c, fr)
        assert_open_equal(e, ref, 0, "a fresh store after all of it")
    finally:
        e.close()


# ---------------------------------------------------------------------------- 9. HybridPipeline and e2e --inventory_evidence
def test_hybrid_pipeline_and_e2e_evidence(synth_models, cls_state, tmp_path, capsys):
    import csv
    import json

    from PIL import Image

    from litepi import HybridPipeline, e2e
    p, b = synth_models["v1"]
    cls_file = str(tmp_path / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in cls_state.items()}, cls_file)
    calls = clip(21, n_calls=3)
    B, size = 2, 64
    tcfg = dict(n_streams=B, max_tracks=64, max_age=0, min_hits=1, iou_match=0.5)
    pipe = HybridPipeline(p, b, cls_file, "shufflenetv2", num_classes=91, precision="fp16", max_batch=4, max_det=32, track=True,
                          track_config=tcfg, inventory=True, evidence={"size": size, "scale": 3.0})
    try:
        for frames in calls:
            pipe.run_batch(list(frames), CONF, IOU, MIN_AREA, stream_ids=list(range(B)))
        signs = pipe.drain_signs(flush=True)
    finally:
        pipe.close()
    assert len(signs) >= 2 and all("evidence" in s and "evidence_window" in s for s in signs)
    n = 0
    for s in signs:
        if s["evidence"] is None:
            assert s["evidence_window"] is None
            continue
        x, y, w, h = s["evidence_window"]
        assert 16 <= w <= PW and 16 <= h <= PH and 0 <= x <= PW - w and 0 <= y <= PH - h
        want = E.picture(calls[s["best_frame"]][s["stream"]], size, s["evidence_window"])
        assert s["evidence"].shape == (size, size, 3) and s["evidence"].tobytes() == want.tobytes(), s["track_id"]
        n += 1
    assert n >= 2
    # the CLI: one sequence of raw BGR frames, one stream
    seq = np.concatenate([c[:1] for c in calls] * 2)   # 6 frames
    seq.tofile(tmp_path / "clip.bgr")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(91)}))
    out = tmp_path / "out"
    argv = ["--detector_param", p, "--detector_bin", b, "--classifier", cls_file, "--clf_arch", "shufflenetv2", "--labels", str(tmp_path),
            "--classes", str(classes), "--batch_images", "3", "--max_det", "32", "--raw_frames", str(tmp_path / "clip.bgr"), "--frame_size",
            f"{PW}x{PH}", "--output", str(out), "--track", "--track_iou", "0.4", "--track_max_age", "0", "--track_min_hits", "1", "--inventory",
            "--inventory_evidence", "48", "--inventory_evidence_scale", "2.5", "--benchmark_conf", str(CONF), "--yolo_conf", "0.04", "--warmup", "1"]
    assert e2e.main(argv) == 0
    capsys.readouterr()
    run = out / "v1+shufflenetv2"
    with open(run / "signs.csv", newline="") as f:
        rows = list(csv.reader(f))
    cols = e2e.SIGNS_CSV_COLUMNS + e2e.EVIDENCE_CSV_COLUMNS
    assert tuple(rows[0]) == cols and rows[0][-4:] == ["evidence_x", "evidence_y", "evidence_w", "evidence_h"] and len(rows) > 2
    n_png = 0
    for r in rows[1:]:
        rec = dict(zip(cols, r))
        png = run / f"signs/sign_{rec['stream']}_{rec['track_id']}_evidence.png"
        if rec["evidence_w"] == "":
            assert not png.exists()
            continue
        win = tuple(int(rec[k]) for k in e2e.EVIDENCE_CSV_COLUMNS)
        want = E.picture(seq[int(rec["best_frame"])], 48, win)
        assert np.asarray(Image.open(png)).tobytes() == np.ascontiguousarray(want[:, :, ::-1]).tobytes(), rec["track_id"]
        n_png += 1
    assert n_png >= 1
