"""GPU tests of class distributions (include/litepi.h, lp_topk), everything through the C-ABI: the select kernel
alone against the NumPy restatement of the rule (tests/topk_ref.py), the argument errors, the tracker's distribution vote
against TrackerTopkRef, the records every pipeline family leaves, and run_batch_device -> track_topk_device end to end.

The tracker scenes are tracking_ref.make_scene(seed, 16, 58, n_frames = 60) for the seeds of TRACK_CASES (0, 1, 2, 3, 5): on
each, and on the three-stream interleavings used here, the oracle keeps every match decision more than 1e-4 away from
flipping (tests/test_topk_cpu.py checks that without a device, as tests/test_gpu_tracking.py demands of its scenes)."""
import ctypes as C

import numpy as np
import pytest
import torch

import topk_ref as K
import tracking_ref as R

pytestmark = pytest.mark.gpu

NCS = (1, 3, 58, 64, 65, 130)
KS = (1, 3, 8)
NC_TRACK = 58
SCENE_FRAMES = 60
MARGIN = 1e-4
# seed, k, vote_decay, n_streams: max_det = 16, max_tracks = 8
TRACK_CASES = [(0, 1, 1.0, 1), (1, 3, 0.9, 1), (2, 8, 1.0, 3), (3, 3, 0.9, 3), (5, 8, 0.9, 1), (1, 1, 1.0, 3)]
SCENE_SEEDS = sorted({c[0] for c in TRACK_CASES})


def stream_ids(n, n_streams):
    return None if n_streams == 1 else np.array([(2 * b + b // 5) % n_streams for b in range(n)], np.int32)


def tracker_case(i):
    """scene, records, configuration and the reference's run of TRACK_CASES[i] (no device)"""
    seed, k, decay, n_streams = TRACK_CASES[i]
    dets, counts = R.make_scene(seed, 16, NC_TRACK, n_frames=SCENE_FRAMES)
    ids = stream_ids(len(counts), n_streams)
    topk = K.random_records(seed + 100, dets.shape, NC_TRACK, k)
    cfg = dict(max_tracks=8, n_streams=n_streams, vote_decay=decay)
    ref = K.TrackerTopkRef(max_det=16, num_classes=NC_TRACK, **cfg)
    want = ref.track_topk(dets, counts, topk, ids)
    return dets, counts, ids, topk, cfg, ref, want


def assert_records_equal(got, want, counts, tag):
    for b, n in enumerate(counts):
        g, w = got[b, :n], want[b, :n]
        if g.tobytes() != w.tobytes():
            for name in g.dtype.names:
                bad = np.flatnonzero(g[name].view(np.int32) != w[name].view(np.int32))
                assert len(bad) == 0, f"{tag}: frame {b}, field {name}, record {bad[0]}: got {g[name][bad[0]]!r}, want {w[name][bad[0]]!r}"


def assert_snapshot_equal(got, want, tag):
    assert (got["next_id"], got["overflow"]) == (want["next_id"], want["overflow"]), tag
    assert got["tracks"].tobytes() == want["tracks"].tobytes(), f"{tag}: track states differ"
    assert got["acc"].shape == want["acc"].shape and got["acc"].tobytes() == want["acc"].tobytes(), f"{tag}: vote accumulators differ"


def run_topk_calls(eng, dets, counts, topk, chunk, ids=None):
    outs = [eng.track_topk(dets[i:i + chunk], counts[i:i + chunk], topk[i:i + chunk], None if ids is None else ids[i:i + chunk])
            for i in range(0, len(counts), chunk)]
    return np.concatenate(outs, 0)


# ---------------------------------------------------------------------------- 1. the select kernel alone
@pytest.mark.parametrize("nc", NCS)
def test_select_kernel_equals_the_rule(nc):
    from litepi import Engine
    MB, MD = 2, 16
    eng = Engine(precision="fp16", max_batch=MB, max_det=MD, num_classes=nc)
    try:
        dists = list(K.distributions(nc).values())
        rng = np.random.default_rng(nc)
        for k in KS:
            eng.topk_enable(k)
            # the sentinel: every record of both frames named, holding the head of a ramp
            sent_p = np.tile(np.linspace(1.0, 2.0, nc, dtype=np.float32) / np.float32(2 * nc), (MB * MD, 1))
            every = np.arange(MB * MD)
            for R_, B in ((0, 1), (0, 2), (1, 1), (1, 2), (5, 1), (5, 2), (16, 1), (32, 2)):
                sentinel = eng.test_topk(sent_p, every // MD, every % MD, MB)
                assert not K.is_empty(sentinel).any()
                z = rng.normal(0, 3, (R_, nc))
                probs = np.exp(z - z.max(1, keepdims=True))
                probs = (probs / probs.sum(1, keepdims=True)).astype(np.float32)
                for r in range(R_):   # the named distributions take the first rows
                    if r < len(dists):
                        probs[r] = dists[r]
                where = rng.permutation(B * MD)[:R_]   # a random injective map ROI -> (frame, slot)
                img, slot = where // MD, where % MD
                got = eng.test_topk(probs, img, slot, B)
                want = K.empty_records((B, MD))
                for r in range(R_):
                    want[img[r], slot[r]] = K.select(probs[r], k)
                assert got.shape == (B, MD) and got.tobytes() == want.tobytes(), (nc, k, R_, B)
                assert K.is_empty(got).sum() == B * MD - R_
                both = eng.topk_read(MB)
                assert both[:B].tobytes() == want.tobytes() and both[B:].tobytes() == sentinel[B:].tobytes(), \
                    f"nc {nc} k {k} R {R_} B {B}: the records of frames >= B must be left alone"
                dev, kk = eng.topk_buffer()
                assert dev != 0 and dev % 16 == 0 and kk == k
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 2. errors
def test_errors_leave_the_handle_usable():
    from litepi import Engine, _ffi
    MB, MD, NC = 2, 16, 58
    eng = Engine(precision="fp16", max_batch=MB, max_det=MD, num_classes=NC)
    lib, h = eng.lib, eng._h
    ip, fp, vp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_void_p
    dev = torch.device("cuda", 0)
    try:
        rec = np.zeros((MB, MD), dtype=_ffi.TOPK_DTYPE)
        probs = np.full((MB * MD + 1, NC), 1.0 / NC, np.float32)
        idx = np.arange(MB * MD + 1, dtype=np.int32)
        img, slot = (idx // MD % MB).astype(np.int32), (idx % MD).astype(np.int32)

        def test_topk(R_, B, im=img, sl=slot):
            return lib.lp_test_topk(h, probs.ctypes.data_as(fp), R_, im.ctypes.data_as(ip), sl.ctypes.data_as(ip), B, rec.ctypes.data)
        for k in (-1, 9):
            assert lib.lp_topk_enable(h, k) == _ffi.LP_ERR_ARG
        p, kk = vp(), C.c_int()
        assert lib.lp_topk_buffer(h, C.byref(p), C.byref(kk)) == _ffi.LP_ERR_STATE
        assert lib.lp_topk_read(h, rec.ctypes.data, 1) == _ffi.LP_ERR_STATE
        assert test_topk(1, 1) == _ffi.LP_ERR_STATE
        eng.topk_enable(3)
        addr, _ = eng.topk_buffer()
        d = torch.zeros(MB * MD * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(MB, dtype=torch.int32, device=dev)
        t = torch.zeros(MB * MD * 32, dtype=torch.uint8, device=dev)
        hd, hc, ht = np.zeros((MB, MD), dtype=_ffi.DET_DTYPE), np.zeros(MB, np.int32), np.zeros((MB, MD), dtype=_ffi.TRACK_DTYPE)

        def dev_call(topk, B):
            return lib.lp_track_topk_device(h, vp(d.data_ptr()), vp(c.data_ptr()), vp(topk) if topk else None, B, None, vp(t.data_ptr()))

        def host_call(topk, B):
            return lib.lp_track_topk(h, hd.ctypes.data, hc.ctypes.data_as(ip), topk, B, None, ht.ctypes.data)
        assert dev_call(addr, 1) == _ffi.LP_ERR_STATE and host_call(rec.ctypes.data, 1) == _ffi.LP_ERR_STATE   # no tracker
        eng.tracker_create(max_tracks=8)
        assert dev_call(0, 1) == _ffi.LP_ERR_ARG and dev_call(addr + 8, 1) == _ffi.LP_ERR_ARG
        assert host_call(None, 1) == _ffi.LP_ERR_ARG
        for B in (0, MB + 1):
            assert dev_call(addr, B) == _ffi.LP_ERR_ARG and host_call(rec.ctypes.data, B) == _ffi.LP_ERR_ARG
            assert lib.lp_topk_read(h, rec.ctypes.data, B) == _ffi.LP_ERR_ARG
            assert test_topk(1, B) == _ffi.LP_ERR_ARG
        assert eng.cfg.max_rois in (0, MB * MD) and test_topk(MB * MD + 1, MB) == _ffi.LP_ERR_ARG
        bad = img.copy()
        bad[2] = MB
        assert test_topk(5, MB, im=bad) == _ffi.LP_ERR_ARG
        bad = slot.copy()
        bad[2] = MD
        assert test_topk(5, MB, sl=bad) == _ffi.LP_ERR_ARG
        bad[2] = -1
        assert test_topk(5, MB, sl=bad) == _ffi.LP_ERR_ARG
        assert lib.lp_last_error()
        # nothing was enqueued, nothing is live, and the handle still works
        assert len(eng.tracker_snapshot(0)["tracks"]) == 0
        got = eng.test_topk(probs[:3], img[:3], slot[:3], MB)
        assert got[0, :3].tobytes() == np.array([K.select(probs[0], 3)] * 3).tobytes() and K.is_empty(got).sum() == MB * MD - 3
        dets, counts, topk, _, Bc = K.acd_against_b(MD)
        assert eng.track_topk(dets[:2], counts[:2], topk[:2])[1, 0]["voted_class"] == Bc
        assert dev_call(addr, MB) == 0
        eng.synchronize()
        eng.topk_enable(0)
        assert lib.lp_topk_buffer(h, C.byref(p), C.byref(kk)) == _ffi.LP_ERR_STATE
        eng.topk_enable(8)
        assert eng.topk_buffer() == (addr, 8), "the buffer's address is stable until lp_destroy"
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 3. the tracker's distribution vote
@pytest.fixture(scope="module")
def engines():
    """handles without models (the tracker needs none), keyed by max_det"""
    from litepi import Engine
    es = {md: Engine(precision="fp16", max_batch=64, max_det=md, num_classes=NC_TRACK) for md in (16, 300)}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("i", range(len(TRACK_CASES)), ids=[f"seed{s}-k{k}-d{d}-s{n}" for s, k, d, n in TRACK_CASES])
def test_distribution_vote_equals_reference(engines, i):
    dets, counts, ids, topk, cfg, ref, want = tracker_case(i)
    assert ref.min_margin > MARGIN, f"case {TRACK_CASES[i]}: a match decision has margin {ref.min_margin:.3g}"
    eng = engines[16]
    eng.tracker_create(**cfg)
    got = run_topk_calls(eng, dets, counts, topk, 7, ids)
    assert_records_equal(got, want, counts, str(TRACK_CASES[i]))
    for s in range(cfg["n_streams"]):
        assert_snapshot_equal(eng.tracker_snapshot(s), ref.snapshot(s), f"{TRACK_CASES[i]} stream {s}")
    assert (want["voted_class"] >= 0).any()


@pytest.mark.parametrize("k, decay", [(1, 1.0), (3, 0.9), (8, 1.0)])
def test_large_frames_read_their_record_from_the_same_index(engines, k, decay):
    """max_det = 300, max_tracks = 256 and a frame of 280 detections: beyond the 256 records the kernel caches in LDS.  A grid
    of boxes drifting two pixels a frame: exact ties, no margin needed, the arithmetic is the same on both sides."""
    rng = np.random.default_rng(17 + k)
    md, T = 300, 6
    dets = np.zeros((T, md), dtype=R.DET_DTYPE)
    counts = np.array([120, 280, 280, 90, 280, 300], np.int32)
    gx, gy = np.meshgrid(np.arange(20), np.arange(15))
    for t in range(T):
        x1 = (gx.ravel() * 60 + 2 * t).astype(np.float32)
        y1 = (gy.ravel() * 45).astype(np.float32)
        d = dets[t]
        d["x1"], d["y1"], d["x2"], d["y2"] = x1, y1, x1 + 40, y1 + 30
        d["det_conf"] = rng.choice(np.array([0.3, 0.5, 0.5, 0.7], np.float32), md)
        d["det_class"] = np.arange(md) % 2   # by grid position: the same from frame to frame
        d["cls_class"], d["cls_conf"] = -1, 0  # not read by the distribution vote
        dets[t] = d[rng.permutation(md)]          # births go by record order: the late records must not always be the overflow
    topk = K.random_records(k, dets.shape, NC_TRACK, k)
    cfg = dict(max_tracks=256, vote_decay=decay)
    ref = K.TrackerTopkRef(max_det=md, num_classes=NC_TRACK, **cfg)
    want = ref.track_topk(dets, counts, topk)
    eng = engines[md]
    eng.tracker_create(**cfg)
    got = run_topk_calls(eng, dets, counts, topk, 4)
    assert_records_equal(got, want, counts, f"k {k}")
    assert_snapshot_equal(eng.tracker_snapshot(0), ref.snapshot(0), f"k {k}")
    late = want[2, 256:280]
    assert (late["voted_class"] >= 0).sum() >= 10, "records past the LDS cache must vote"


def test_hand_made_records(engines):
    NC, MD = NC_TRACK, 16
    box = (100.0, 80.0, 140.0, 120.0, 0.9, 0)
    cases = {
        "a class named twice, a track born voting": [[(4, 0.5), (4, 0.25)]],
        "cls[0] = -1 with a valid cls_class": [[(-1, 0.5), (3, 0.25)]] * 2,
        "cls[0] >= num_classes": [[(NC, 0.5), (3, 0.25)]] * 2,
        "cls[0] far out of range": [[(1 << 30, 0.5)], [(-(1 << 31), 0.5)]],
        "an out-of-range entry at j = 2": [[(1, 0.5), (3, 0.25), (NC, 0.125), (5, 0.0625)]] * 3,
        "vote, no vote, vote": [[(1, 0.5), (3, 0.25)], [(-1, 0.9)], [(3, 0.5), (1, 0.25), (3, 0.125)]],
        "eight entries": [[(c, 0.5 / (c + 1)) for c in range(8)]] * 2,
    }
    eng = engines[MD]
    for name, frames in cases.items():
        dets = np.zeros((len(frames), MD), dtype=R.DET_DTYPE)
        topk = K.empty_records((len(frames), MD))
        for f, entries in enumerate(frames):
            dets[f, 0] = box + (2, 0.7)   # a valid lp_det::cls_class that must not be read
            for j, (c, p) in enumerate(entries):
                topk[f, 0]["cls"][j], topk[f, 0]["prob"][j] = c, p
        counts = np.ones(len(frames), np.int32)
        cfg = dict(max_tracks=4, vote_decay=0.5)
        ref = K.TrackerTopkRef(max_det=MD, num_classes=NC, **cfg)
        want = ref.track_topk(dets, counts, topk)
        eng.tracker_create(**cfg)
        got = eng.track_topk(dets, counts, topk)
        assert_records_equal(got, want, counts, name)
        assert_snapshot_equal(eng.tracker_snapshot(0), ref.snapshot(0), name)
        assert want[0, 0]["flags"] & R.BORN
    assert want[1, 0]["voted_class"] == 0   # the last case votes


def test_one_entry_records_equal_lp_track_on_the_device(engines):
    eng = engines[16]
    for seed, decay in ((0, 1.0), (2, 0.9)):
        dets, counts = R.make_scene(seed, 16, NC_TRACK, n_frames=SCENE_FRAMES)
        ids = stream_ids(len(counts), 3)
        cfg = dict(max_tracks=8, n_streams=3, vote_decay=decay)
        one = K.one_entry_records(dets, NC_TRACK)
        eng.tracker_create(**cfg)
        a = np.concatenate([eng.track(dets[i:i + 7], counts[i:i + 7], ids[i:i + 7]) for i in range(0, len(counts), 7)], 0)
        snaps = [eng.tracker_snapshot(s) for s in range(3)]
        eng.tracker_create(**cfg)   # the twin: a fresh tracker
        b = run_topk_calls(eng, dets, counts, one, 7, ids)
        assert_records_equal(b, a, counts, f"seed {seed}")
        for s in range(3):
            assert_snapshot_equal(eng.tracker_snapshot(s), snaps[s], f"seed {seed} stream {s}")
        assert (a["voted_class"] >= 0).any()


def test_either_call_may_feed_the_tracker_from_frame_to_frame(engines):
    eng = engines[16]
    dets, counts = R.make_scene(3, 16, NC_TRACK, n_frames=SCENE_FRAMES)
    topk = K.random_records(9, dets.shape, NC_TRACK, 3)
    cfg = dict(max_tracks=8, vote_decay=0.9)
    ref = K.TrackerTopkRef(max_det=16, num_classes=NC_TRACK, **cfg)
    eng.tracker_create(**cfg)
    for b in range(len(counts)):
        s = slice(b, b + 1)
        if b % 2:
            got, want = eng.track(dets[s], counts[s]), ref.track(dets[s], counts[s])
        else:
            got, want = eng.track_topk(dets[s], counts[s], topk[s]), ref.track_topk(dets[s], counts[s], topk[s])
        assert_records_equal(got, want, counts[s], f"frame {b}")
    assert ref.min_margin > MARGIN
    assert_snapshot_equal(eng.tracker_snapshot(0), ref.snapshot(0), "alternating")


def test_distribution_vote_finds_b(engines):
    eng = engines[16]
    dets, counts, topk, A, Bc = K.acd_against_b(16)
    eng.tracker_create(max_tracks=8)
    assert eng.track(dets, counts)[2, 0]["voted_class"] == A
    eng.tracker_create(max_tracks=8)
    got = eng.track_topk(dets, counts, topk)
    want = K.TrackerTopkRef(max_det=16, num_classes=NC_TRACK, max_tracks=8).track_topk(dets, counts, topk)
    assert got[2, 0]["voted_class"] == Bc and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------- 4. the pipeline
CONF, IOU, MIN_AREA = 0.25, 0.45, 50
N_CALLS, N_FRAMES, NC_PIPE, TOPK = 6, 2, 91, 5


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
def clip():
    rng = np.random.default_rng(77)
    return moving_patch(rng.integers(0, 256, (N_FRAMES, 640, 640, 3), dtype=np.uint8), rng)


@pytest.fixture(scope="module")
def models(tmp_path_factory, clip):
    """a seeded v1 detector whose class bias is shifted so that on the first and the last call's frames at least three anchors
    pass conf 0.25 with a margin of 0.1 in the logit, measured with the device's own scores (as tests/test_gpu_inventory.py),
    and a seeded classifier"""
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    d = tmp_path_factory.mktemp("topk_models")
    sd = random_shufflenet_state(NC_PIPE, seed=3)
    cls_file = str(d / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, cls_file)
    every = [f for k in (0, N_CALLS - 1) for f in clip[k]]
    p, b = str(d / "v1.param"), str(d / "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=4321, cls_bias=0.0)
    e = Engine(precision="fp16", max_batch=len(every), max_det=300, num_classes=NC_PIPE)
    try:
        e.load_detector(p, b)
        lb = np.stack([e.test_letterbox(f)[0] for f in every])
        s = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64), axis=1)[:, ::-1]
    finally:
        e.close()
    third = s[:, 2].min()
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - (np.log(third / (1 - third)) - 0.1)))
    return {"cls": sd, "cls_file": cls_file, "v1": (p, b)}


def _engine(models, prec, max_batch=4, max_rois=0):
    from litepi import Engine
    e = Engine(precision=prec, max_batch=max_batch, max_det=300, num_classes=NC_PIPE, max_rois=max_rois)
    e.load_detector(*models["v1"])
    e.load_classifier(models["cls"])
    return e


def check_records(dets, counts, topk, nc, tag):
    """(b): every classified record's top-k starts with the record's arg-max and is a sorted head of a distribution; every other
    record of the frames is empty.  Returns the number of classified records."""
    n_cls = 0
    for b in range(len(counts)):
        for i in range(dets.shape[1]):
            d, t = dets[b, i], topk[b, i]
            if i < counts[b] and d["cls_class"] >= 0:
                n_cls += 1
                m = min(TOPK, nc)
                assert t["cls"][0] == d["cls_class"] and t["prob"][0].tobytes() == d["cls_conf"].tobytes(), f"{tag}: record ({b}, {i})"
                assert (np.diff(t["prob"][:m]) <= 0).all() and (t["prob"][:m] >= 0).all(), f"{tag}: record ({b}, {i}) is not sorted"
                assert len(set(t["cls"][:m].tolist())) == m and (t["cls"][:m] >= 0).all() and (t["cls"][:m] < nc).all()
                assert (t["cls"][m:] == -1).all() and (t["prob"][m:] == 0).all()
                assert t["prob"].astype(np.float64).sum() <= 1 + 1e-5
            else:
                assert K.is_empty(np.array([t]))[0], f"{tag}: record ({b}, {i}) must be empty"
    return n_cls


def prob_tolerance(models, prec, crops_bgr):
    """Twice the bound tests/test_gpu_classifier.py documents for the precision, turned into probabilities.  That bound is on
    log p against the float64 module, computed on the ROIs at hand: fp16, 2 x the error of the path's fp16-storage emulation;
    fp32, 10 x the gap between the float32 and the float64 module.  |log p - log p_ref| <= b means |p - p_ref| <=
    p_ref (e^b - 1) <= e^b - 1, and two device paths within that of the oracle are within 2 (e^b - 1) of each other."""
    from oracle import shufflenet_ref as S
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in models["cls"].items()}
    module = S.ShuffleNetV2(NC_PIPE)
    missing = module.load_state_dict(sd, strict=False)   # the seeded state has no num_batches_tracked counters
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys)
    module, x = module.eval(), S.input_batch(crops_bgr)
    ref = S.logp_module(module, x)
    if prec == "fp16":
        b = 2 * np.abs(S.folded_logp(sd, crops_bgr, "fused") - ref).max()
    else:
        b = 10 * np.abs(S.logp_module(module, x, torch.float32) - ref).max()
    return 2 * float(np.expm1(b))


@pytest.fixture(scope="module", params=["fp32", "fp16"])
def piped(request, models, clip):
    """one handle per precision (max_batch 4, 2 frames, k = 5): the device step with top-k off, on and off again -- records,
    launch lists, graph counters -- and what the other checks need of the `on` state"""
    from litepi._ffi import DET_DTYPE
    prec = request.param
    dev = torch.device("cuda", 0)
    eng = _engine(models, prec)
    B = N_FRAMES
    x = torch.from_numpy(clip[0]).to(dev)
    d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
    c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
    out = {"prec": prec, "eng": eng, "x": x, "d": d, "c": c, "states": []}

    def step():
        eng.run_batch_device(x.data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())

    def fetch():
        eng.synchronize()
        return d.cpu().numpy().copy(), c.cpu().numpy().copy()
    try:
        for k in (0, TOPK, 0):
            eng.topk_enable(k)
            for _ in range(3):   # eager, capture, replay
                step()
            st = {"k": k, "bytes": tuple(a.tobytes() for a in fetch())}
            if k:
                before = eng.graph_stats()
                for _ in range(10):
                    step()
                eng.synchronize()
                st["stats"] = (before, eng.graph_stats())
                st["bytes10"] = tuple(a.tobytes() for a in fetch())
                st["topk"] = eng.topk_read(B)
                st["rois"] = eng.debug_rois()
                st["overflow"] = eng.roi_overflow()
            eng.profile_next(True)
            step()
            eng.synchronize()
            st["launches"] = [(r["name"], r["layer"]) for r in eng.profile_read()]
            st["bytes_profiled"] = tuple(a.tobytes() for a in fetch())
            if k:
                st["topk_profiled"] = eng.topk_read(B)
            out["states"].append(st)
        dn, cn = fetch()
        out["dets"], out["counts"] = dn.view(DET_DTYPE).reshape(B, 300), cn[:B]
        eng.topk_enable(TOPK)
        yield out
    finally:
        eng.close()


def test_records_are_the_same_off_on_and_off_again(piped):   # (a)
    off, on, off2 = piped["states"]
    assert off["bytes"] == on["bytes"] == off2["bytes"], "lp_det records or counts differ with top-k on"
    assert on["bytes10"] == on["bytes"] and on["bytes_profiled"] == on["bytes"] and off["bytes_profiled"] == off["bytes"]
    assert piped["counts"].min() >= 1


def test_topk_records_of_the_device_step(piped):   # (b)
    on = piped["states"][1]
    n = check_records(piped["dets"], piped["counts"], on["topk"], NC_PIPE, piped["prec"])
    assert n == piped["counts"].sum() >= 2 and on["overflow"] == (n, n)
    assert on["topk_profiled"].tobytes() == on["topk"].tobytes(), "the eager profiled step leaves other records than the replayed one"


def test_topk_against_the_full_distribution(piped, models):   # (c)
    eng, on = piped["eng"], piped["states"][1]
    crops, img, slot = on["rois"]
    assert len(img) == piped["counts"].sum()
    bgr = [np.ascontiguousarray(cr[:, :, ::-1]) for cr in crops]
    assert eng.test_roi_resize(bgr).tobytes() == crops.tobytes(), "a 64 x 64 crop must pass the ROI resize unchanged"
    ids, full = eng.classify(bgr)
    tol = prob_tolerance(models, piped["prec"], bgr)
    print(f"TOPK {piped['prec']}: tol {tol:.3e}")
    assert 0 < tol < 0.5
    worst = 0.0
    for r in range(len(img)):   # no record is exempt
        t = on["topk"][img[r], slot[r]]
        m = min(TOPK, NC_PIPE)
        err = np.abs(t["prob"][:m].astype(np.float64) - full[r, t["cls"][:m]].astype(np.float64))
        worst = max(worst, float(err.max()))
        assert (err <= tol).all(), f"ROI {r}: top-k probabilities off by {err.max():.3e} > {tol:.3e}"
        rest = np.delete(full[r].astype(np.float64), t["cls"][:m])
        assert (rest <= float(t["prob"][m - 1]) + tol).all(), f"ROI {r}: a class outside the record beats its last entry"
    print(f"TOPK {piped['prec']}: max |prob - full| {worst:.3e} over {len(img)} ROIs")


def test_unclassified_kept_records_are_empty(piped, models):   # (d)
    from litepi._ffi import DET_DTYPE
    dev = torch.device("cuda", 0)
    B = N_FRAMES
    eng = _engine(models, piped["prec"], max_rois=1)
    try:
        eng.topk_enable(TOPK)
        d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        eng.run_batch_device(piped["x"].data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
        classified, kept = eng.roi_overflow()
        assert classified == 1 and kept >= 2
        dets, counts = d.cpu().numpy().view(DET_DTYPE).reshape(B, 300), c.cpu().numpy()[:B]
        topk = eng.topk_read(B)
        assert check_records(dets, counts, topk, NC_PIPE, "max_rois = 1") == 1
        _, img, slot = eng.debug_rois()
        assert len(img) == 1 and not K.is_empty(topk[img[0], slot[0]][None])[0]
        assert K.is_empty(topk).sum() == B * 300 - 1 and (dets["cls_class"][np.arange(300)[None, :] < counts[:, None]] < 0).sum() == kept - 1
    finally:
        eng.close()


def test_views_and_host_calls_index_records_by_frame(piped, clip):   # (e)
    from litepi._ffi import DET_DTYPE
    eng, B = piped["eng"], N_FRAMES
    dev = torch.device("cuda", 0)
    d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
    c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
    eng.run_views_device(piped["x"].data_ptr(), B, 640, 640, ["full", (128, 128, 384, 384)], CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
    topk = eng.topk_read(B)
    dets, counts = d.cpu().numpy().view(DET_DTYPE).reshape(B, 300), c.cpu().numpy()[:B]
    assert check_records(dets, counts, topk, NC_PIPE, "views") >= 2 and counts.min() >= 1
    hd, hc, _, timing = eng.run_batch(list(clip[0]), CONF, IOU, MIN_AREA)
    topk = eng.topk_read(B)
    assert check_records(hd[:B], hc[:B], topk, NC_PIPE, "host") == piped["counts"].sum()
    used = np.arange(300)[None, :] < piped["counts"][:, None]
    assert (hc[:B] == piped["counts"]).all() and hd[:B][used].tobytes() == piped["dets"][used].tobytes()
    assert topk.tobytes() == piped["states"][1]["topk"].tobytes(), "the host call leaves other records than the device call"
    assert timing.t_classification > 0


def test_repeated_steps_are_replays(piped):   # (f)
    before, after = piped["states"][1]["stats"]
    assert after["replays"] - before["replays"] == 10 and after["eager"] == before["eager"] and after["captures"] == before["captures"]


def test_launch_lists(piped):   # (g)
    off, on, off2 = (s["launches"] for s in piped["states"])
    assert off == off2 and len(off) > 10, "a handle switched on and off again must run the launches it ran before"
    assert not any("topk" in name for name, _ in off)
    extra = [x for x in on if x[0].startswith("topk")]
    assert [x for x in on if not x[0].startswith("topk")] == off, "top-k on must add launches only"
    assert 1 <= len(extra) <= 2 and {n for n, _ in extra} <= {"topk_clear", "topk_select"} and "topk_select" in {n for n, _ in extra}


# ---------------------------------------------------------------------------- 5. end to end
def test_run_batch_device_into_track_topk_device(models, clip):
    from litepi import HybridPipeline
    from litepi._ffi import DET_DTYPE, TRACK_DTYPE
    dev = torch.device("cuda", 0)
    B, k = N_FRAMES, 3
    tcfg = dict(n_streams=B, max_tracks=64, max_age=0, min_hits=2, iou_match=0.5, vote_decay=0.9)
    sid = np.arange(B, dtype=np.int32)
    eng = _engine(models, "fp16")
    ref = K.TrackerTopkRef(max_det=300, num_classes=NC_PIPE, **tcfg)
    want_all = []
    try:
        eng.topk_enable(k)
        eng.tracker_create(**tcfg)
        addr, _ = eng.topk_buffer()
        d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        t = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        for call, frames in enumerate(clip):   # six calls of two streams' frames
            x = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
            eng.run_batch_device(x.data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
            eng.track_topk_device(d.data_ptr(), c.data_ptr(), addr, B, t.data_ptr(), sid)   # no synchronise in between
            topk = eng.topk_read(B)   # synchronises
            counts = c.cpu().numpy()[:B].copy()
            dets = d.cpu().numpy().view(DET_DTYPE).reshape(B, 300).copy()
            tracks = t.cpu().numpy().view(TRACK_DTYPE).reshape(B, 300)
            want = ref.track_topk(dets, counts, topk, sid)
            assert_records_equal(tracks, want, counts, f"call {call}")
            assert counts.min() >= 1
            want_all.append((dets, counts, topk, want))
        for s in range(B):
            assert_snapshot_equal(eng.tracker_snapshot(s), ref.snapshot(s), f"stream {s}")
        assert max(w["hits"][b, :cn[b]].max() for _, cn, _, w in want_all for b in range(B)) >= 3, "no track lived three frames"
    finally:
        eng.close()
    # the same capacity as the handle above: the detector's launches are planned by max_batch, and another plan rounds otherwise
    pipe = HybridPipeline(*models["v1"], models["cls_file"], "shufflenetv2", num_classes=NC_PIPE, precision="fp16", max_batch=4,
                          topk=k, track=True, track_config=tcfg, track_vote="distribution")
    try:
        for call, frames in enumerate(clip):
            dets, counts, topk, want = want_all[call]
            outs = pipe.run_batch(list(frames), CONF, IOU, MIN_AREA, stream_ids=sid)
            for b, (res, _) in enumerate(outs):
                assert len(res) == counts[b]
                for i, r in enumerate(res):
                    assert r["cls_topk"][0] == (r["cls_class"], r["cls_conf"]) and 1 <= len(r["cls_topk"]) <= k
                    assert [cc for cc, _ in r["cls_topk"]] == topk[b, i]["cls"][:len(r["cls_topk"])].tolist()
                    assert r["det_conf"] == float(dets[b, i]["det_conf"]), f"call {call} ({b}, {i}): the host call found another record"
                    assert r["track_cls"] == want[b, i]["voted_class"] and r["track_id"] == want[b, i]["track_id"], f"call {call} ({b}, {i})"
    finally:
        pipe.close()
