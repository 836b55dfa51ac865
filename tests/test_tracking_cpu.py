"""CPU tests of sign tracking: hand-worked cases of the rule's NumPy restatement (tests/tracking_ref.py), lp_track_config_check
(pure host, like lp_tile_grid and lp_frame_layout), the exported symbols and the --track refusals of the CLI.  No device."""
import ctypes as C

import numpy as np
import pytest

import tracking_ref as R


def frame(recs, max_det=8):
    """recs: (x1, y1, x2, y2[, det_conf, det_class, cls_class, cls_conf]) -> one frame of lp_det records + its count"""
    d = np.zeros(max_det, dtype=R.DET_DTYPE)
    for i, r in enumerate(recs):
        d[i] = tuple(r) + (0.9, 0, -1, 0.0)[len(r) - 4:]
    return d, len(recs)


def feed(ref, recs, max_det=8, stream=0):
    d, n = frame(recs, max_det)
    return ref.track(d[None], [n], [stream])[0][:n]


BOX = (100.0, 100.0, 140.0, 140.0)


# ---------------------------------------------------------------------------- identity
def test_id_survives_max_age_missed_frames_and_is_replaced_after_one_more():
    for gap, same in ((3, True), (4, False)):
        ref = R.TrackerRef(max_det=8, max_age=3, motion=0)
        first = feed(ref, [BOX])
        assert (first["track_id"][0], first["hits"][0], first["age"][0], first["flags"][0]) == (1, 1, 0, R.BORN)
        for _ in range(gap):
            assert len(feed(ref, [])) == 0
        again = feed(ref, [BOX])
        if same:
            assert (again["track_id"][0], again["hits"][0], again["age"][0], again["flags"][0]) == (1, 2, gap + 1, 0)
        else:
            assert (again["track_id"][0], again["hits"][0], again["age"][0], again["flags"][0]) == (2, 1, 0, R.BORN)
            assert ref.snapshot()["next_id"] == 3


def test_constant_velocity_reacquires_after_a_gap_where_a_static_prediction_loses():
    def run(motion):
        ref = R.TrackerRef(max_det=8, max_age=5, motion=motion)
        ids = []
        for t in range(12):
            if 5 <= t < 9:   # four frames without a detection while the sign moves on by 15 px per frame
                feed(ref, [])
                continue
            x = 100.0 + 15.0 * t
            ids.append(int(feed(ref, [(x, 100.0, x + 40.0, 140.0)])["track_id"][0]))
        return ids
    assert run(1) == [1] * 8
    assert run(0) == [1] * 5 + [2] * 3   # 75 px on a 40 px box: IoU 0 against the last box


def test_velocity_and_prediction_values():
    ref = R.TrackerRef(max_det=8, motion=1)
    feed(ref, [(10.0, 20.0, 50.0, 60.0)])
    feed(ref, [])
    feed(ref, [(16.0, 20.0, 58.0, 64.0)])   # dt = 2
    t = ref.snapshot()["tracks"][0]
    assert (t["vx1"], t["vy1"], t["vx2"], t["vy2"]) == (3.0, 0.0, 4.0, 2.0)
    assert (t["hits"], t["missed"], t["age"]) == (2, 0, 2)


def test_confirmed_flag_and_hits():
    ref = R.TrackerRef(max_det=8, min_hits=3)
    flags = [int(feed(ref, [BOX])["flags"][0]) for _ in range(4)]
    assert flags == [R.BORN, 0, R.CONFIRMED, R.CONFIRMED]


# ---------------------------------------------------------------------------- votes
def label_sequence(n=40, seed=5, right=7, p=0.7):
    rng = np.random.default_rng(seed)
    lab = [right if rng.random() < p else int(rng.integers(0, 58)) for _ in range(n)]
    assert 0.6 <= sum(1 for v in lab if v == right) / n <= 0.8
    return lab


def test_vote_over_a_70_percent_correct_label_sequence():
    ref = R.TrackerRef(max_det=8)
    for lab in label_sequence():
        out = feed(ref, [BOX + (0.9, 0, lab, 0.5)])
    assert out["voted_class"][0] == 7 and out["track_id"][0] == 1
    assert out["vote_weight"][0] == np.float32(20.0) and 0.6 <= out["voted_conf"][0] <= 0.8


def test_no_vote_until_a_classified_detection():
    ref = R.TrackerRef(max_det=8)
    out = feed(ref, [BOX + (0.9, 0, -1, 0.0)])
    assert (out["voted_class"][0], out["voted_conf"][0], out["vote_weight"][0]) == (-1, 0.0, 0.0)
    out = feed(ref, [BOX + (0.9, 0, 12, 0.25)])
    assert (out["voted_class"][0], out["voted_conf"][0], out["vote_weight"][0]) == (12, 1.0, 0.25)
    out = feed(ref, [BOX + (0.9, 0, 99, 0.5)])   # outside 0..num_classes-1: not a vote
    assert (out["voted_class"][0], out["vote_weight"][0]) == (12, 0.25)


def test_vote_decay_lets_a_late_label_change_win():
    def run(decay):
        ref = R.TrackerRef(max_det=8, vote_decay=decay)
        for lab in [3] * 10 + [4] * 5:
            out = feed(ref, [BOX + (0.9, 0, lab, 0.5)])
        return int(out["voted_class"][0])
    assert run(1.0) == 3   # 5.0 against 2.5
    assert run(0.7) == 4   # the ten early votes have decayed to 0.5 * (0.7^5 + .. + 0.7^14) < 0.5 * (1 + .. + 0.7^4)


def test_vote_arithmetic_is_fp32_in_the_stated_order():
    ref = R.TrackerRef(max_det=8, vote_decay=0.9)
    f = np.float32
    acc3 = acc5 = wsum = f(0)
    for lab, conf in ((3, 0.3), (5, 0.7), (3, 0.45)):
        feed(ref, [BOX + (0.9, 0, lab, conf)])
        acc3, acc5, wsum = f(acc3 * f(0.9)), f(acc5 * f(0.9)), f(f(wsum * f(0.9)) + f(conf))
        if lab == 3:
            acc3 = f(acc3 + f(conf))
        else:
            acc5 = f(acc5 + f(conf))
    s = ref.snapshot()
    assert s["acc"][0, 3] == acc3 and s["acc"][0, 5] == acc5 and s["tracks"]["wsum"][0] == wsum


# ---------------------------------------------------------------------------- table, gate, ties
def test_full_table_leaves_detections_untracked_and_counts_the_overflow():
    ref = R.TrackerRef(max_det=8, max_tracks=2)
    boxes = [(50.0 * i, 0.0, 50.0 * i + 30.0, 30.0) for i in range(4)]
    out = feed(ref, boxes)
    assert out["track_id"].tolist() == [1, 2, 0, 0] and out["slot"].tolist() == [0, 1, -1, -1]
    assert out["voted_class"].tolist()[2:] == [-1, -1] and out["hits"].tolist() == [1, 1, 0, 0]
    assert ref.snapshot()["overflow"] == 2
    out = feed(ref, boxes)
    assert out["track_id"].tolist() == [1, 2, 0, 0] and ref.snapshot()["overflow"] == 4


def test_new_conf_keeps_weak_detections_from_starting_a_track():
    ref = R.TrackerRef(max_det=8, new_conf=0.5)
    out = feed(ref, [BOX + (0.4,), (300.0, 300.0, 340.0, 340.0, 0.5)])
    assert out["track_id"].tolist() == [0, 1]
    assert ref.snapshot()["overflow"] == 0   # below new_conf is not an overflow


def test_class_gate():
    for gate, expect in ((1, 2), (0, 1)):
        ref = R.TrackerRef(max_det=8, class_gate=gate)
        feed(ref, [BOX + (0.9, 0)])
        assert feed(ref, [BOX + (0.9, 1)])["track_id"][0] == expect


def test_freed_slot_is_reused_in_the_same_frame_and_lowest_slot_first():
    ref = R.TrackerRef(max_det=8, max_tracks=2, max_age=0)
    feed(ref, [BOX, (300.0, 300.0, 340.0, 340.0)])
    out = feed(ref, [(600.0, 300.0, 640.0, 340.0), (300.0, 300.0, 340.0, 340.0)])   # track 1 is lost: its slot 0 is free again
    assert out["track_id"].tolist() == [3, 2] and out["slot"].tolist() == [0, 1]


def test_tie_rules():
    # two tracks with the same predicted box: the detection takes the lower slot; two detections of equal det_conf: the lower
    # record index is matched first and takes it
    ref = R.TrackerRef(max_det=8, motion=0)
    first = feed(ref, [BOX, BOX])
    assert first["slot"].tolist() == [0, 1]
    out = feed(ref, [BOX + (0.8,), BOX + (0.8,)])
    assert out["slot"].tolist() == [0, 1] and out["track_id"].tolist() == [1, 2]
    # a higher det_conf goes first whatever its record index
    out = feed(ref, [BOX + (0.5,), BOX + (0.8,)])
    assert out["slot"].tolist() == [1, 0]
    # equal votes: the lower class
    ref = R.TrackerRef(max_det=8)
    feed(ref, [BOX + (0.9, 0, 9, 0.5)])
    assert feed(ref, [BOX + (0.9, 0, 4, 0.5)])["voted_class"][0] == 4
    # births in record order, not score order
    ref = R.TrackerRef(max_det=8)
    assert feed(ref, [BOX + (0.3,), (300.0, 300.0, 340.0, 340.0, 0.9)])["track_id"].tolist() == [1, 2]


def test_nan_never_matches():
    ref = R.TrackerRef(max_det=8)
    feed(ref, [BOX])
    out = feed(ref, [(float("nan"), 100.0, 140.0, 140.0)])
    assert out["track_id"][0] == 2


def test_streams_are_independent_and_reset_keeps_the_ids_counting():
    ref = R.TrackerRef(max_det=8, n_streams=2)
    assert feed(ref, [BOX], stream=0)["track_id"][0] == 1
    assert feed(ref, [BOX], stream=1)["track_id"][0] == 1
    assert feed(ref, [BOX], stream=1)["hits"][0] == 2
    ref.reset(1)
    assert feed(ref, [BOX], stream=1)["track_id"][0] == 2
    assert feed(ref, [BOX], stream=0)["hits"][0] == 2


def test_conf_key_order():
    conf = np.array([0.5, 0.25, 1.0, 0.0, -1.0, 0.5], np.float32)
    keys = R.conf_keys(conf)
    assert sorted(range(6), key=lambda i: (-int(keys[i]), i)) == [2, 0, 5, 1, 3, 4]


def test_scene_generator_is_deterministic_and_within_bounds():
    d1, c1 = R.make_scene(11, max_det=16)
    d2, c2 = R.make_scene(11, max_det=16)
    assert d1.tobytes() == d2.tobytes() and c1.tolist() == c2.tolist()
    assert 40 <= len(c1) <= 200 and 0 <= c1.min() and c1.max() <= 16 and c1.sum() > 0
    assert (d1["cls_class"] == -1).any() and (d1["cls_class"] >= 0).any()


# ---------------------------------------------------------------------------- the library's host-only entry point
def test_track_config_check_on_the_loaded_library():
    from litepi import _ffi
    from litepi.backend import track_config, track_config_check

    assert C.sizeof(_ffi.LpTrack) == 32 and C.sizeof(_ffi.LpTrackState) == 64 and C.sizeof(_ffi.LpTrackConfig) == 64
    assert np.dtype(_ffi.TRACK_DTYPE).itemsize == 32 and np.dtype(_ffi.TRACK_STATE_DTYPE).itemsize == 64
    assert _ffi.TRACK_DTYPE == R.TRACK_DTYPE and _ffi.TRACK_STATE_DTYPE == R.TRACK_STATE_DTYPE
    d = track_config()
    assert track_config_check(d) == _ffi.LP_OK
    assert {k: getattr(d, k) for k in R.DEFAULTS if k != "max_tracks"} == pytest.approx({k: v for k, v in R.DEFAULTS.items() if k != "max_tracks"})
    assert track_config_check(None) == _ffi.LP_ERR_ARG
    good = [dict(n_streams=1024), dict(max_tracks=256), dict(max_tracks=1), dict(iou_match=0.0), dict(max_age=0), dict(vote_decay=1.0),
            dict(new_conf=-1.0), dict(class_gate=0, motion=0)]
    for kw in good:
        assert track_config_check(track_config(**kw)) == _ffi.LP_OK, kw
    bad = [dict(n_streams=0), dict(n_streams=1025), dict(max_tracks=0), dict(max_tracks=257), dict(iou_match=-0.01), dict(iou_match=1.0),
           dict(iou_match=float("nan")), dict(max_age=-1), dict(min_hits=0), dict(new_conf=float("nan")), dict(vote_decay=0.0),
           dict(vote_decay=1.01), dict(vote_decay=float("nan")), dict(class_gate=2), dict(class_gate=-1), dict(motion=2), dict(motion=-1)]
    for kw in bad:
        assert track_config_check(track_config(**kw)) == _ffi.LP_ERR_ARG, kw
    for i in range(7):
        c = track_config()
        c.reserved[i] = 1
        assert track_config_check(c) == _ffi.LP_ERR_ARG, i
    with pytest.raises(TypeError):
        track_config(max_trakcs=3)


def test_symbols_are_exported():
    from litepi import _ffi

    lib = _ffi.load_library()
    names = ["lp_track_default_config", "lp_track_config_check", "lp_tracker_create", "lp_tracker_destroy", "lp_tracker_reset",
             "lp_track_device", "lp_track", "lp_tracker_snapshot"]
    for s in names:
        assert s in _ffi.SYMBOLS
        getattr(lib, s)
    assert lib.lp_version() == 310


# ---------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("extra, word", [([], "--raw_frames"), (["--raw_frames", "f.yuv", "--frame_size", "64x64", "--num_samples", "3"], "--num_samples"),
                                         (["--raw_frames", "f.yuv", "--frame_size", "64x64", "--gpus", "2"], "--gpus")])
def test_cli_refuses_track_without_a_sequence(extra, word, monkeypatch):
    from litepi import backend, e2e

    def no_model(*a, **k):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(backend, "HybridPipeline", no_model)
    args = e2e.build_parser().parse_args(["--track"] + extra)
    with pytest.raises(SystemExit) as ei:
        e2e.check_frame_args(args)
    assert word in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        e2e.run_evaluation(args)
    assert word in str(ei.value)


def test_cli_refuses_track_under_a_multi_process_launch(tmp_path, monkeypatch):
    from litepi import backend, e2e

    def no_model(*a, **k):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(backend, "HybridPipeline", no_model)
    np.zeros((2, 64, 64, 3), np.uint8).tofile(tmp_path / "clip.bgr")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    args = e2e.build_parser().parse_args(["--track", "--raw_frames", str(tmp_path / "clip.bgr"), "--frame_size", "64x64"])
    with pytest.raises(SystemExit) as ei:
        e2e.run_evaluation(args)
    assert "WORLD_SIZE" in str(ei.value)


def test_cli_track_arguments():
    from litepi import e2e

    a = e2e.build_parser().parse_args([])
    assert (a.track, a.track_iou, a.track_max_age, a.track_min_hits) == (False, 0.3, 5, 3)
    a = e2e.build_parser().parse_args(["--track", "--track_iou", "0.4", "--track_max_age", "2", "--track_min_hits", "1"])
    assert (a.track, a.track_iou, a.track_max_age, a.track_min_hits) == (True, 0.4, 2, 1)
    assert e2e.TRACKS_CSV_COLUMNS[:2] == ("frame", "track_id") and len(e2e.TRACKS_CSV_COLUMNS) == 13
