"""CPU tests of the sign inventory's rule (tests/inventory_ref.py) and of the library's host-only entry points.

1. mirror: an inventory that sees only the records of each frame keeps the tracker's table in step: the open (slot, id) set and
   the missed counters equal TrackerRef.snapshot after every frame, slots freed and reused within one frame included;
2. every logged sign equals a brute-force pass over the whole record stream;
3. the log: unique ids, min_hits, split invariance, duplicate / out-of-range slots, overflow order and `dropped`;
4. lp_inventory_config_check, struct sizes, exported symbols, CLI refusals."""
import ctypes as C

import numpy as np
import pytest

import inventory_ref as V
import tracking_ref as R

NC = 58
# (seed, max_tracks, max_age, max_det): scenes of 72-176 frames
MIRROR = [(0, 4, 0, 16), (7000, 4, 0, 300), (1000, 4, 3, 16), (2000, 64, 3, 300), (5000, 256, 5, 16), (11000, 64, 0, 300), (30001, 256, 3, 16)]


def tracked_scene(seed, max_det, **tcfg):
    dets, counts = R.make_scene(seed, max_det=max_det, num_classes=NC)
    trk = R.TrackerRef(max_det=max_det, num_classes=NC, **tcfg)
    return dets, counts, trk


# ---------------------------------------------------------------------------- 1. mirror
@pytest.mark.parametrize("seed, T, age, md", MIRROR)
def test_inventory_mirrors_the_tracker_table(seed, T, age, md):
    tcfg = dict(max_tracks=T, max_age=age)
    dets, counts, trk = tracked_scene(seed, md, **tcfg)
    assert 72 <= len(counts) <= 176
    inv = V.InventoryRef(md, tcfg)
    reuse_frames = 0
    for f in range(len(counts)):
        before = {s: i for s, i, _ in inv.open_state(0)}
        tracks = trk.track(dets[f:f + 1], counts[f:f + 1])
        inv.feed(dets[f:f + 1], tracks, counts[f:f + 1])
        snap = trk.snapshot(0)["tracks"]
        got = inv.open_state(0)
        assert [(s, i) for s, i, _ in got] == list(zip(snap["slot"].tolist(), snap["track_id"].tolist())), f"frame {f}"
        assert [m for _, _, m in got] == snap["missed"].tolist(), f"frame {f}"
        reuse_frames += any(s in before and before[s] != i for s, i, _ in got)
    if T == 4:
        assert reuse_frames > 0, "no slot was freed and reused within one frame"
    if (seed, T, age, md) == (0, 4, 0, 16):
        assert reuse_frames == 33
    if (seed, T, age, md) == (7000, 4, 0, 300):
        assert reuse_frames == 23


# ---------------------------------------------------------------------------- 2. brute force
def brute_force(dets, counts, tracks, best):
    """per id over the whole record stream: first / last frame, first-maximum best sighting, the last sighting's vote"""
    out = {}
    for f in range(len(counts)):
        for i in range(counts[f]):
            t, d = tracks[f, i], dets[f, i]
            if t["track_id"] <= 0:
                continue
            q = V.quality(d, best)
            s = out.setdefault(int(t["track_id"]), dict(first=f, best_q=q, best=(f, i)))
            if q > s["best_q"]:
                s["best_q"], s["best"] = q, (f, i)
            s["last"], s["final"] = f, t
    return out


@pytest.mark.parametrize("best", [V.BEST_AREA, V.BEST_DET_CONF, V.BEST_CLS_CONF])
@pytest.mark.parametrize("seed, T, age, md", [(0, 4, 0, 16), (2000, 64, 3, 300), (30001, 256, 3, 16)])
def test_logged_signs_equal_a_brute_force_pass(seed, T, age, md, best):
    tcfg = dict(max_tracks=T, max_age=age, min_hits=2)
    dets, counts, trk = tracked_scene(seed, md, **tcfg)
    tracks = trk.track(dets, counts)
    inv = V.InventoryRef(md, tcfg, dict(best=best, max_signs=1 << 20))
    inv.feed(dets, tracks, counts)
    done, _, dropped = inv.drain()
    assert dropped == 0 and not (done["flags"] & V.FLUSHED).any()
    inv.flush()
    rest, _, _ = inv.drain()
    assert len(rest) and (rest["flags"] & V.FLUSHED).all()
    signs = np.concatenate([done, rest])
    want = brute_force(dets, counts, tracks, best)
    assert len(set(signs["track_id"].tolist())) == len(signs), "an id was logged twice"
    assert set(signs["track_id"].tolist()) == {i for i, s in want.items() if s["final"]["hits"] >= 2}
    for s in signs:
        w = want[int(s["track_id"])]
        f, i = w["best"]
        assert (s["first_frame"], s["last_frame"], s["best_frame"]) == (w["first"], w["last"], f)
        assert s["best_quality"].tobytes() == w["best_q"].tobytes()
        assert [s[k] for k in ("x1", "y1", "x2", "y2", "det_class")] == [dets[f, i][k] for k in ("x1", "y1", "x2", "y2", "det_class")]
        assert [s[k] for k in ("hits", "voted_class", "voted_conf", "vote_weight")] == \
               [w["final"][k] for k in ("hits", "voted_class", "voted_conf", "vote_weight")]
    # a finished sign is logged in the frame its track is freed: last_frame + max_age + 1 frames are over by then
    assert (done["last_frame"] + age + 1 <= len(counts) - 1).all()


# ---------------------------------------------------------------------------- 3. the log
def test_split_invariance_and_min_hits():
    tcfg = dict(max_tracks=16, max_age=2)
    dets, counts, trk = tracked_scene(4242, 16, **tcfg)
    tracks = trk.track(dets, counts)
    results = []
    for chunk in (len(counts), 1, 7):
        inv = V.InventoryRef(16, tcfg, dict(min_hits=1))
        for i in range(0, len(counts), chunk):
            inv.feed(dets[i:i + chunk], tracks[i:i + chunk], counts[i:i + chunk])
        inv.flush()
        results.append(inv.drain()[0].tobytes())
    assert results[0] == results[1] == results[2]
    every = np.frombuffer(results[0], dtype=V.SIGN_DTYPE)
    for mh, tracker_mh in ((0, 3), (0, 9), (9, 1), (20, 3)):   # 0 = the tracker's min_hits
        thr = mh or tracker_mh
        inv = V.InventoryRef(16, dict(tcfg, min_hits=tracker_mh), dict(min_hits=mh))
        inv.feed(dets, tracks, counts)
        inv.flush()
        signs = inv.drain()[0]
        assert signs.tobytes() == every[every["hits"] >= thr].tobytes()
        assert len(signs) > 0 and (thr < 9 or len(signs) < len(every)), thr


def _records(md, frames):
    """frames: lists of (track_id, slot, hits, x2) -> dets, tracks, counts"""
    dets = np.zeros((len(frames), md), dtype=R.DET_DTYPE)
    tracks = np.zeros((len(frames), md), dtype=R.TRACK_DTYPE)
    counts = np.array([len(f) for f in frames], np.int32)
    for b, f in enumerate(frames):
        for i, (tid, slot, hits, x2) in enumerate(f):
            dets[b, i] = (0, 0, x2, 10, 0.5, 1, 3, 0.7)
            tracks[b, i] = (tid, slot, hits, 0, 3, 0.9, 1.0, 1)
    return dets, tracks, counts


def test_duplicate_and_out_of_range_slots():
    # slot 9 and -1 are out of range (max_tracks = 4) and ignored; of two records naming slot 1 the lower index counts
    frames = [[(5, 9, 1, 10), (6, -1, 1, 10), (7, 1, 1, 20), (8, 1, 1, 30), (0, 2, 1, 10)]]
    inv = V.InventoryRef(8, dict(max_tracks=4, max_age=0, min_hits=1))
    inv.feed(*_records(8, frames))
    assert inv.open_state(0) == [(1, 7, 0)]
    assert inv.open(0)["x2"].tolist() == [20.0]
    # the same slot with another id closes the entry and opens a new one in the same frame
    inv.feed(*_records(8, [[(8, 1, 1, 30)]]))
    signs, _, _ = inv.drain()
    assert signs["track_id"].tolist() == [7] and inv.open_state(0) == [(1, 8, 0)]
    assert (signs["first_frame"][0], signs["last_frame"][0]) == (0, 0) and inv.open(0)["first_frame"].tolist() == [1]


def test_ties_keep_the_earlier_sighting_and_nan_never_replaces():
    d, t, c = _records(8, [[(1, 0, 1, 10)], [(1, 0, 2, 10)], [(1, 0, 3, float("nan"))], [(1, 0, 4, 9)], [(1, 0, 5, 11)]])
    inv = V.InventoryRef(8, dict(max_tracks=4, min_hits=1))
    for f, want in enumerate([0, 0, 0, 0, 4]):
        inv.feed(d[f:f + 1], t[f:f + 1], c[f:f + 1])
        assert inv.open(0)["best_frame"].tolist() == [want]
    d, t, c = _records(8, [[(1, 0, 1, float("nan"))], [(1, 0, 2, 50)]])   # a first sighting is the best whatever its quality
    inv = V.InventoryRef(8, dict(max_tracks=4, min_hits=1))
    inv.feed(d, t, c)
    assert inv.open(0)["best_frame"].tolist() == [0] and np.isnan(inv.open(0)["best_quality"][0])


def test_log_overflow_keeps_the_lowest_slots_and_counts_the_rest():
    first = [[(10 + s, s, 1, 10) for s in range(6)]]
    d, t, c = _records(8, first + [[]])
    inv = V.InventoryRef(8, dict(max_tracks=8, max_age=0, min_hits=1), dict(max_signs=4))
    inv.feed(d, t, c)   # frame 1: all six close in one block, four fit
    signs, _, dropped = inv.drain()
    assert signs["track_id"].tolist() == [10, 11, 12, 13] and dropped == 2
    inv.feed(d, t, c)   # the drain re-armed the log
    signs, _, dropped = inv.drain()
    assert signs["track_id"].tolist() == [10, 11, 12, 13] and dropped == 2 and signs["first_frame"].tolist() == [2] * 4
    inv.feed(d[:1], t[:1], c[:1])
    d2, t2, c2 = _records(8, [[(10, 0, 2, 10), (11, 1, 2, 10), (12, 2, 2, 10)], [(10, 0, 3, 10)], []])
    inv.feed(d2, t2, c2)   # blocks of 3, 2 and 1 signs: 3 fit, then 1 of 2, then none
    signs, _, dropped = inv.drain()
    assert signs["track_id"].tolist() == [13, 14, 15, 11] and dropped == 2


def test_crops_follow_the_best_sighting():
    S = 4
    d, t, c = _records(8, [[(1, 0, 1, 10)], [(1, 0, 2, 20)], [(1, 0, 3, 30)], [(1, 0, 4, 5)]])
    crops = {(b, 0): np.full((S, S, 3), 10 * (b + 1), np.uint8) for b in (0, 1, 3)}   # the sighting of frame 2 has no crop
    inv = V.InventoryRef(8, dict(max_tracks=4, min_hits=1), crop_size=S)
    for f, (flag, val) in enumerate([(1, 10), (1, 20), (0, 0), (0, 0)]):
        inv.feed(d[f:f + 1], t[f:f + 1], c[f:f + 1], crops={(0, 0): crops[(f, 0)]} if (f, 0) in crops else None)
        assert inv.open(0)["flags"].tolist() == [flag]
    inv.flush()
    signs, pix, _ = inv.drain()
    assert signs["flags"].tolist() == [V.FLUSHED] and not pix.any()
    assert V.rois_to_crops(np.arange(3), [0, 1, 1], [2, 0, 5], total=2) == {(0, 2): 0, (1, 0): 1}


# ---------------------------------------------------------------------------- 4. the library's host-only entry points, CLI
def test_inventory_config_check_on_the_loaded_library():
    from litepi import _ffi
    from litepi.backend import inventory_config, inventory_config_check

    assert C.sizeof(_ffi.LpSign) == 64 and C.sizeof(_ffi.LpInventoryConfig) == 64
    assert np.dtype(_ffi.SIGN_DTYPE).itemsize == 64 and _ffi.SIGN_DTYPE == V.SIGN_DTYPE
    assert [n for n, _ in _ffi.LpSign._fields_] == [n for n, _ in _ffi.SIGN_DTYPE]
    assert (_ffi.LP_BEST_AREA, _ffi.LP_BEST_DET_CONF, _ffi.LP_BEST_CLS_CONF) == (V.BEST_AREA, V.BEST_DET_CONF, V.BEST_CLS_CONF)
    assert (_ffi.LP_SIGN_HAS_CROP, _ffi.LP_SIGN_FLUSHED) == (V.HAS_CROP, V.FLUSHED)
    d = inventory_config()
    assert inventory_config_check(d) == _ffi.LP_OK
    assert {k: getattr(d, k) for k in V.INV_DEFAULTS} == V.INV_DEFAULTS
    assert inventory_config_check(None) == _ffi.LP_ERR_ARG
    for kw in (dict(max_signs=1), dict(max_signs=1 << 20), dict(keep_crops=0), dict(best=2), dict(best="cls_conf"), dict(min_hits=7)):
        assert inventory_config_check(inventory_config(**kw)) == _ffi.LP_OK, kw
    for kw in (dict(max_signs=0), dict(max_signs=(1 << 20) + 1), dict(keep_crops=2), dict(keep_crops=-1), dict(best=3), dict(best=-1),
               dict(min_hits=-1)):
        assert inventory_config_check(inventory_config(**kw)) == _ffi.LP_ERR_ARG, kw
    for i in range(12):
        c = inventory_config()
        c.reserved[i] = 1
        assert inventory_config_check(c) == _ffi.LP_ERR_ARG, i
    with pytest.raises(TypeError):
        inventory_config(max_sings=3)
    with pytest.raises(ValueError):
        inventory_config(best="biggest")


def test_symbols_are_exported():
    from litepi import _ffi

    lib = _ffi.load_library()
    for s in ("lp_inventory_default_config", "lp_inventory_config_check", "lp_inventory_create", "lp_inventory_destroy", "lp_inventory_device",
              "lp_inventory", "lp_inventory_flush", "lp_inventory_drain", "lp_inventory_open", "lp_test_set_rois", "lp_debug_rois"):
        assert s in _ffi.SYMBOLS
        getattr(lib, s)
    assert lib.lp_version() == 310


def test_cli_refuses_inventory_without_track(monkeypatch):
    from litepi import backend, e2e

    def no_model(*a, **k):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(backend, "HybridPipeline", no_model)
    args = e2e.build_parser().parse_args(["--inventory", "--raw_frames", "f.yuv", "--frame_size", "64x64"])
    with pytest.raises(SystemExit) as ei:
        e2e.check_frame_args(args)
    assert "--track" in str(ei.value)
    with pytest.raises(SystemExit) as ei:
        e2e.run_evaluation(args)
    assert "--track" in str(ei.value)
    with pytest.raises(SystemExit):   # --inventory does not lift --track's own conditions
        e2e.check_frame_args(e2e.build_parser().parse_args(["--inventory", "--track"]))


def test_cli_inventory_arguments():
    from litepi import e2e

    a = e2e.build_parser().parse_args([])
    assert (a.inventory, a.inventory_best) == (False, "area")
    a = e2e.build_parser().parse_args(["--track", "--inventory", "--inventory_best", "cls_conf"])
    assert (a.inventory, a.inventory_best) == (True, "cls_conf")
    with pytest.raises(SystemExit):
        e2e.build_parser().parse_args(["--inventory_best", "largest"])
    assert e2e.SIGNS_CSV_COLUMNS[:2] == ("stream", "track_id") and len(e2e.SIGNS_CSV_COLUMNS) == 15
