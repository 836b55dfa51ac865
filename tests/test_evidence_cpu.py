"""CPU tests of the evidence store's rule (tests/evidence_ref.py) and of the library's host-only entry points.

1. lp_evidence_window on the loaded library == the NumPy restatement, bit for bit, over random and adversarial boxes;
2. inside the frame the window is the focus plan's placement with side_min = 16, margin = scale and no border;
3. lp_evidence_config_check, struct size, exported symbols;
4. the CLI and HybridPipeline refuse the option without what it needs;
5. the reference on itself: a slot closed and reused in one call, a best improved three times, a crops = 0 call."""
import ctypes as C

import numpy as np
import pytest

import evidence_ref as E
import focus_ref
import inventory_ref as V
import tracking_ref as R

F = np.float32
SIZES = [(16, 16), (48, 80), (97, 131), (1080, 1920)]


def boxes_for(H, W, rng, n=3000):
    """random boxes, then boxes on every edge and corner, larger than the frame, 1-pixel, empty, negative, NaN and +-inf"""
    c = rng.uniform(-0.2, 1.2, (n, 2)) * (W, H)
    s = np.exp(rng.uniform(np.log(0.5), np.log(3.0 * max(H, W)), (n, 2)))
    b = np.concatenate([c - s / 2, c + s / 2], 1)
    b[: n // 4] = np.round(b[: n // 4])            # integer corners: centres on .0 and .5
    b[n // 4: n // 2] = np.round(b[n // 4: n // 2] * 2) / 2
    hard = []
    for x1, x2 in ((0, 7), (W - 7, W), (0, W), (-5, 3), (W - 3, W + 5), (W / 2 - 0.5, W / 2 + 0.5)):
        for y1, y2 in ((0, 7), (H - 7, H), (0, H), (-5, 3), (H - 3, H + 5), (H / 2 - 0.5, H / 2 + 0.5)):
            hard.append((x1, y1, x2, y2))
    hard += [(-W, -H, 2 * W, 2 * H), (-1e6, -1e6, 1e6, 1e6), (3, 3, 4, 4), (W - 1, H - 1, W, H), (0, 0, 1, 1),
             (5, 5, 5, 9), (5, 5, 9, 5), (9, 5, 5, 9), (5, 9, 9, 5), (0, 0, 0, 0), (-3, -3, -1, -1), (W + 1, H + 1, W + 3, H + 3),
             (np.nan, 1, 5, 5), (1, np.nan, 5, 5), (1, 1, np.nan, 5), (1, 1, 5, np.nan), (np.nan,) * 4,
             (-np.inf, 1, 5, 5), (1, 1, np.inf, 5), (-np.inf, -np.inf, np.inf, np.inf), (np.inf, 1, np.inf, 5), (1, -np.inf, 5, np.inf),
             (1, 1, 1 + 1e-30, 5), (1e30, 1e30, 3e38, 3e38), (-3e38, 1, 3e38, 5)]
    return np.concatenate([b, np.array(hard, dtype=np.float64)]).astype(np.float32)


# ---------------------------------------------------------------------------- 1. the window on the loaded library
@pytest.mark.parametrize("H, W", SIZES + [(15, 200), (200, 15), (1, 1)])
@pytest.mark.parametrize("scale", [1.0, 2.0, 3.7, 16.0])
def test_window_equals_reference(H, W, scale):
    from litepi.backend import evidence_config, evidence_window

    cfg = evidence_config(scale=scale)
    rng = np.random.default_rng(H * 7 + W + int(scale * 10))
    n_has = 0
    for box in boxes_for(H, W, rng, 3000 if (H, W) in SIZES else 300):
        got = evidence_window(cfg, H, W, box)
        want = E.window(F(scale), H, W, box)
        assert got == want, f"{W}x{H} scale {scale} box {box.tolist()}: library {got}, reference {want}"
        (x, y, w, h), has = got
        n_has += has
        if has:
            assert 16 <= w <= W and 16 <= h <= H and 0 <= x <= W - w and 0 <= y <= H - h
        else:
            assert (x, y, w, h) == (0, 0, 0, 0)
    assert (n_has > 0) == (H >= 16 and W >= 16)


def test_window_arguments():
    from litepi import _ffi
    from litepi.backend import evidence_config

    lib = _ffi.load_library()
    cfg, box, win, has = evidence_config(), (C.c_float * 4)(1, 1, 9, 9), (C.c_int * 4)(), C.c_int()
    assert lib.lp_evidence_window(C.byref(cfg), 64, 64, box, win, C.byref(has)) == _ffi.LP_OK and has.value == 1
    assert list(win) == [0, 0, 16, 16]
    assert lib.lp_evidence_window(None, 64, 64, box, win, C.byref(has)) == _ffi.LP_ERR_ARG
    assert lib.lp_evidence_window(C.byref(cfg), 0, 64, box, win, C.byref(has)) == _ffi.LP_ERR_ARG
    assert lib.lp_evidence_window(C.byref(cfg), 64, 64, None, win, C.byref(has)) == _ffi.LP_ERR_ARG
    assert lib.lp_evidence_window(C.byref(evidence_config(scale=0.5)), 64, 64, box, win, C.byref(has)) == _ffi.LP_ERR_ARG


# ---------------------------------------------------------------------------- 2. the focus plan's placement
@pytest.mark.parametrize("H, W", SIZES[1:])
@pytest.mark.parametrize("scale", [1.0, 2.0, 5.5])
def test_window_is_the_focus_placement(H, W, scale):
    rng = np.random.default_rng(H + W)
    fr = focus_ref.FocusRef(640, slots=1, side_min=16, side_max=E.SIDE_MAX, margin=scale, small_px=1e30, border=0, sweep=0, motion=0)
    n = 0
    for _ in range(400):
        x1, y1 = F(rng.uniform(0, W - 1)), F(rng.uniform(0, H - 1))
        x2, y2 = F(rng.uniform(x1, W)), F(rng.uniform(y1, H))
        if not (x2 > x1 and y2 > y1):
            continue
        t = focus_ref.make_tracks([dict(slot=0, x1=x1, y1=y1, x2=x2, y2=y2, vx1=0, vy1=0, vx2=0, vy2=0, hits=1, missed=0)])
        placed = fr.frame(t, 0, H, W, {"cursor": 0, "unserved": 0})[0]
        win, has = E.window(F(scale), H, W, (x1, y1, x2, y2))
        assert has and tuple(int(v) for v in placed) == win, ((x1, y1, x2, y2), placed, win)
        n += 1
    assert n > 300


# ---------------------------------------------------------------------------- 3. configuration and symbols
def test_evidence_config_check_on_the_loaded_library():
    from litepi import _ffi
    from litepi.backend import evidence_config, evidence_config_check

    assert C.sizeof(_ffi.LpEvidenceConfig) == 32
    assert _ffi.LP_SIGN_HAS_EVIDENCE == E.HAS_EVIDENCE == 4
    d = evidence_config()
    assert (d.size, d.scale) == (E.EV_DEFAULTS["size"], E.EV_DEFAULTS["scale"]) and evidence_config_check(d) == _ffi.LP_OK
    assert evidence_config_check(None) == _ffi.LP_ERR_ARG
    for kw in (dict(size=32), dict(size=256), dict(size=48), dict(scale=1.0), dict(scale=16.0), dict(size=64, scale=3.5)):
        assert evidence_config_check(evidence_config(**kw)) == _ffi.LP_OK, kw
    for kw in (dict(size=16), dict(size=272), dict(size=0), dict(size=-128), dict(size=40), dict(size=100), dict(scale=0.99), dict(scale=16.5),
               dict(scale=0.0), dict(scale=-2.0), dict(scale=float("nan")), dict(scale=float("inf"))):
        assert evidence_config_check(evidence_config(**kw)) == _ffi.LP_ERR_ARG, kw
    for i in range(6):
        c = evidence_config()
        c.reserved[i] = 1
        assert evidence_config_check(c) == _ffi.LP_ERR_ARG, i
    with pytest.raises(TypeError):
        evidence_config(sise=3)


def test_symbols_are_exported():
    from litepi import _ffi

    lib = _ffi.load_library()
    for s in ("lp_evidence_default_config", "lp_evidence_config_check", "lp_evidence_window", "lp_evidence_create", "lp_evidence_destroy",
              "lp_inventory_drain_evidence", "lp_evidence_open", "lp_test_set_frames"):
        assert s in _ffi.SYMBOLS
        getattr(lib, s)
    assert lib.lp_version() == 310


# ---------------------------------------------------------------------------- 4. refusals
def test_cli_refuses_evidence_without_inventory(monkeypatch):
    from litepi import backend, e2e

    def no_model(*a, **k):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(backend, "HybridPipeline", no_model)
    base = ["--raw_frames", "f.yuv", "--frame_size", "64x64", "--inventory_evidence", "64"]
    for extra in ([], ["--track"], ["--inventory"]):
        args = e2e.build_parser().parse_args(base + extra)
        with pytest.raises(SystemExit) as ei:
            e2e.check_frame_args(args)
        assert "--track" in str(ei.value)
        with pytest.raises(SystemExit):
            e2e.run_evaluation(args)
    for bad in (["--inventory_evidence", "40"], ["--inventory_evidence", "512"], ["--inventory_evidence", "64", "--inventory_evidence_scale", "0.5"],
                ["--inventory_evidence_scale", "2"]):
        with pytest.raises(SystemExit) as ei:
            e2e.check_frame_args(e2e.build_parser().parse_args(["--track", "--inventory", "--raw_frames", "f.yuv", "--frame_size", "64x64"] + bad))
        assert "--inventory_evidence" in str(ei.value)
    a = e2e.build_parser().parse_args([])
    assert (a.inventory_evidence, a.inventory_evidence_scale) == (None, None)
    a = e2e.build_parser().parse_args(["--inventory_evidence", "96", "--inventory_evidence_scale", "3"])
    assert (a.inventory_evidence, a.inventory_evidence_scale) == (96, 3.0)
    assert e2e.EVIDENCE_CSV_COLUMNS == ("evidence_x", "evidence_y", "evidence_w", "evidence_h")


def test_pipeline_refuses_evidence_without_inventory(monkeypatch):
    from litepi import backend

    def no_handle(*a, **k):
        raise AssertionError("a handle was created before the arguments were checked")
    monkeypatch.setattr(backend, "Engine", no_handle)
    for kw in (dict(evidence=128), dict(evidence=128, track=True), dict(evidence={"size": 64}, track=True),
               dict(evidence=40, track=True, inventory=True), dict(evidence={"size": 64, "scale": 40.0}, track=True, inventory=True),
               dict(evidence=64, track=True, inventory=dict(keep_crops=0))):
        with pytest.raises(ValueError) as ei:
            backend.HybridPipeline("d.param", "d.bin", "c.pth", "shufflenetv2", **kw)
        assert "evidence" in str(ei.value), kw


# ---------------------------------------------------------------------------- 5. the reference on itself
MD = 4


def records(frames):
    """frames: a list of [(slot, track_id, (x1, y1, x2, y2))]"""
    dets, trk = np.zeros((len(frames), MD), dtype=R.DET_DTYPE), np.zeros((len(frames), MD), dtype=R.TRACK_DTYPE)
    counts = np.zeros(len(frames), np.int32)
    for b, recs in enumerate(frames):
        counts[b] = len(recs)
        for i, (slot, tid, box) in enumerate(recs):
            dets[b, i]["x1"], dets[b, i]["y1"], dets[b, i]["x2"], dets[b, i]["y2"] = box
            trk[b, i]["track_id"], trk[b, i]["slot"], trk[b, i]["hits"] = tid, slot, 1
    return dets, trk, counts


def frames_of(n, H=48, W=80, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def test_reference_slot_closed_and_reused_in_one_call():
    fr = frames_of(3)
    ref = E.EvidenceRef(MD, dict(max_tracks=2, max_age=0, min_hits=1), ev_cfg=dict(size=32))
    d, t, c = records([[(0, 1, (10, 10, 20, 20))], [(0, 2, (40, 20, 52, 30))], [(0, 2, (40, 20, 50, 28))]])
    ref.feed(d, t, c, frames=fr)
    signs, _, pics, wins, _ = ref.drain_evidence()
    assert signs["track_id"].tolist() == [1] and signs["flags"].tolist() == [E.HAS_EVIDENCE]
    w0 = E.window(F(2), 48, 80, (10, 10, 20, 20))[0]
    assert wins[0].tolist() == list(w0) and pics[0].tobytes() == E.picture(fr[0], 32, w0).tobytes()
    op, ow = ref.open_evidence(0)
    w1 = E.window(F(2), 48, 80, (40, 20, 52, 30))[0]
    assert ow.tolist() == [list(w1)] and op[0].tobytes() == E.picture(fr[1], 32, w1).tobytes()


def test_reference_best_improved_three_times_in_one_call():
    fr = frames_of(4, seed=1)
    ref = E.EvidenceRef(MD, dict(max_tracks=2, max_age=0, min_hits=1), ev_cfg=dict(size=32))
    boxes = [(10, 10, 14, 14), (10, 10, 16, 16), (10, 10, 18, 18), (10, 10, 20, 20)]
    d, t, c = records([[(1, 7, b)] for b in boxes])
    ref.feed(d, t, c, frames=fr)
    assert ref.rendered == 4
    ref.flush()
    signs, _, pics, wins, _ = ref.drain_evidence()
    w = E.window(F(2), 48, 80, boxes[3])[0]
    assert signs["best_frame"].tolist() == [3] and signs["flags"].tolist() == [E.HAS_EVIDENCE | V.FLUSHED]
    assert wins[0].tolist() == list(w) and pics[0].tobytes() == E.picture(fr[3], 32, w).tobytes()


def test_reference_crops_0_call_clears_the_flag():
    fr = frames_of(2, seed=2)
    ref = E.EvidenceRef(MD, dict(max_tracks=2, max_age=0, min_hits=1), ev_cfg=dict(size=32))
    d, t, c = records([[(0, 3, (10, 10, 14, 14)), (1, 4, (30, 30, 44, 44))], [(0, 3, (10, 10, 20, 20)), (1, 4, (30, 30, 40, 40))]])
    ref.feed(d[:1], t[:1], c[:1], frames=fr[:1])
    assert (ref.open(0)["flags"] & E.HAS_EVIDENCE).tolist() == [4, 4]
    ref.feed(d[1:], t[1:], c[1:], frames=None)   # entry 3 takes a new best without frames; entry 4 keeps its old best and picture
    assert (ref.open(0)["flags"] & E.HAS_EVIDENCE).tolist() == [0, 4]
    pics, wins = ref.open_evidence(0)
    assert not pics[0].any() and wins[0].tolist() == [0, 0, 0, 0]
    w = E.window(F(2), 48, 80, (30, 30, 44, 44))[0]
    assert wins[1].tolist() == list(w) and pics[1].tobytes() == E.picture(fr[0], 32, w).tobytes()
    nan = E.EvidenceRef(MD, dict(max_tracks=2, max_age=0, min_hits=1), ev_cfg=dict(size=32))
    d, t, c = records([[(0, 1, (np.nan, 1, 5, 5)), (1, 2, (9, 9, 9, 12))]])
    nan.feed(d, t, c, frames=fr[:1])
    assert nan.open(0)["flags"].tolist() == [0, 0] and not nan.open_evidence(0)[0].any()
