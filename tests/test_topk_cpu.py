"""CPU tests of class distributions (include/litepi.h, lp_topk): lp_topk_select against the NumPy restatement of the selection
rule (tests/topk_ref.py), the record layout and the exported symbols, the distribution vote's restatement against the tracker's
(one-entry records must change nothing), the refusals of HybridPipeline and the CLI, and the shared comparator header under
sanitizers as a stand-alone program.  No device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import topk_ref as K
import tracking_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lp_topk_enable", "lp_topk_buffer", "lp_topk_read", "lp_topk_select", "lp_track_topk_device", "lp_track_topk", "lp_test_topk")
NCS = (1, 3, 58, 64, 65, 130)
KS = (1, 3, 8)


def _lib():
    from litepi import _ffi
    return _ffi.load_library()


# ---------------------------------------------------------------------------- the selection rule
@pytest.mark.parametrize("nc", NCS)
def test_topk_select_equals_the_rule_bit_for_bit(nc):
    from litepi import backend
    for k in KS:
        for name, p in K.distributions(nc).items():
            got, want = backend.topk_select(p, k), K.select(p, k)
            assert got.tobytes() == want.tobytes(), (nc, k, name, got, want)
            m = min(k, nc)
            assert (got["cls"][m:] == -1).all() and (got["prob"][m:].view(np.uint32) == 0).all()
            assert got["cls"][0] == int(np.argmax(p)) and got["prob"][0].tobytes() == p[np.argmax(p)].tobytes()   # np.argmax: first maximum
            if name == "one_hot":   # the zero ties come out lowest class first
                zeros = [c for c in range(nc) if p[c] == 0][:m - 1]
                assert got["cls"][1:m].tolist() == zeros
            if name == "equal":
                assert got["cls"][:m].tolist() == list(range(m))


def test_topk_select_refuses_bad_arguments():
    from litepi import _ffi
    lib = _lib()
    p = np.full(4, 0.25, np.float32)
    fp = p.ctypes.data_as(C.POINTER(C.c_float))
    out = _ffi.LpTopk()
    assert lib.lp_topk_select(fp, 4, 3, C.byref(out)) == 0 and list(out.cls) == [0, 1, 2, -1, -1, -1, -1, -1]
    for args in ((None, 4, 3, C.byref(out)), (fp, 4, 3, None), (fp, 0, 3, C.byref(out)), (fp, -1, 3, C.byref(out)), (fp, 4, 0, C.byref(out)),
                 (fp, 4, 9, C.byref(out)), (fp, 4, -1, C.byref(out))):
        assert lib.lp_topk_select(*args) == _ffi.LP_ERR_ARG, args[1:3]
        assert lib.lp_last_error()


def test_ref_select_is_the_rule_on_a_hand_case():
    p = np.array([0.1, 0.3, 0.3, 0.05, 0.25], np.float32)
    r = K.select(p, 3)
    assert r["cls"].tolist() == [1, 2, 4, -1, -1, -1, -1, -1]
    assert r["prob"][:3].tobytes() == p[[1, 2, 4]].tobytes() and (r["prob"][3:] == 0).all()
    assert K.is_empty(K.empty_records(3)).all() and not K.is_empty(np.array([r]))[0]


# ---------------------------------------------------------------------------- layout and exports
def test_layout_and_exports():
    from litepi import _ffi
    lib = _lib()
    assert C.sizeof(_ffi.LpTopk) == 64 and np.dtype(_ffi.TOPK_DTYPE).itemsize == 64 and np.dtype(K.TOPK_DTYPE) == np.dtype(_ffi.TOPK_DTYPE)
    assert _ffi.LpTopk.cls.offset == 0 and _ffi.LpTopk.prob.offset == 32 and _ffi.LP_TOPK_MAX == K.TOPK_MAX == 8
    header = open(os.path.join(ROOT, "include", "litepi.h")).read()
    declared = set(re.findall(r"\b(lp_[a-z0-9_]+)\s*\(", header))
    assert "#define LP_TOPK_MAX 8" in header
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/litepi.h"
        assert s in _ffi.SYMBOLS and hasattr(lib, s) and getattr(lib, s).restype is C.c_int
    assert lib.lp_version() == 310 == _ffi.ABI_VERSION


# ---------------------------------------------------------------------------- the distribution vote, ref against ref
def _same(a: dict, b: dict) -> bool:
    return (a["tracks"].tobytes() == b["tracks"].tobytes() and a["acc"].tobytes() == b["acc"].tobytes() and
            (a["next_id"], a["overflow"]) == (b["next_id"], b["overflow"]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("decay", [1.0, 0.9])
def test_one_entry_records_vote_as_the_top1_tracker(seed, decay):
    MD, NC = 16, 58
    dets, counts = R.make_scene(seed, MD, NC, n_frames=60)
    ids = [(b * 2 + b // 5) % 3 for b in range(len(counts))]   # 3 interleaved streams
    cfg = dict(max_tracks=8, n_streams=3, vote_decay=decay)
    base, new = R.TrackerRef(max_det=MD, num_classes=NC, **cfg), K.TrackerTopkRef(max_det=MD, num_classes=NC, **cfg)
    topk = K.one_entry_records(dets, NC)
    for lo in range(0, len(counts), 4):
        a = base.track(dets[lo:lo + 4], counts[lo:lo + 4], ids[lo:lo + 4])
        b = new.track_topk(dets[lo:lo + 4], counts[lo:lo + 4], topk[lo:lo + 4], ids[lo:lo + 4])
        assert a.tobytes() == b.tobytes(), (seed, decay, lo)
    assert (dets["cls_class"] >= 0).any() and (dets["cls_class"] < 0).any()
    for s in range(3):
        assert _same(base.snapshot(s), new.snapshot(s))
    assert sum(len(base.snapshot(s)["tracks"]) for s in range(3)) > 0


def test_either_vote_may_feed_the_same_tracker():
    MD, NC = 16, 58
    dets, counts = R.make_scene(1, MD, NC, n_frames=40)
    topk = K.one_entry_records(dets, NC)
    base, mixed = R.TrackerRef(max_det=MD, num_classes=NC, max_tracks=8), K.TrackerTopkRef(max_det=MD, num_classes=NC, max_tracks=8)
    for b in range(len(counts)):
        a = base.track(dets[b:b + 1], counts[b:b + 1])
        m = mixed.track(dets[b:b + 1], counts[b:b + 1]) if b % 2 else mixed.track_topk(dets[b:b + 1], counts[b:b + 1], topk[b:b + 1])
        assert a.tobytes() == m.tobytes()
    assert _same(base.snapshot(), mixed.snapshot())


def test_distribution_vote_finds_b_where_top1_finds_a():
    dets, counts, topk, A, B = K.acd_against_b(8)
    top1, dist = R.TrackerRef(max_det=8, num_classes=58, max_tracks=4), K.TrackerTopkRef(max_det=8, num_classes=58, max_tracks=4)
    a, d = top1.track(dets, counts)[2, 0], dist.track_topk(dets, counts, topk)[2, 0]
    assert (a["track_id"], a["hits"], d["track_id"], d["hits"]) == (1, 3, 1, 3)
    assert a["voted_class"] == A and abs(a["voted_conf"] - 0.40 / 1.20) < 1e-6 and abs(a["vote_weight"] - 1.20) < 1e-6
    assert d["voted_class"] == B and abs(d["voted_conf"] - 1.05 / 2.25) < 1e-6 and abs(d["vote_weight"] - 2.25) < 1e-6


def test_distribution_vote_hand_cases():
    NC = 10
    box = (100.0, 80.0, 140.0, 120.0, 0.9, 0)

    def run(entries, cls_class=2, frames=1):
        ref = K.TrackerTopkRef(max_det=4, num_classes=NC, max_tracks=2, vote_decay=0.5)
        dets = np.zeros((frames, 4), dtype=R.DET_DTYPE)
        topk = K.empty_records((frames, 4))
        for f in range(frames):
            dets[f, 0] = box + (cls_class, 0.7)
            for j, (c, p) in enumerate(entries):
                topk[f, 0]["cls"][j], topk[f, 0]["prob"][j] = c, p
        out = ref.track_topk(dets, np.ones(frames, np.int32), topk)
        return out[frames - 1, 0], ref.snapshot()
    # a class named twice is added twice; a track that is born votes
    rec, snap = run([(4, 0.5), (4, 0.25)])
    assert rec["flags"] & R.BORN and rec["voted_class"] == 4 and snap["acc"][0, 4] == np.float32(0.75) and rec["vote_weight"] == np.float32(0.75)
    # cls[0] = -1 with a valid lp_det::cls_class: no vote; cls[0] >= num_classes: no vote
    for first in (-1, NC, NC + 5):
        rec, snap = run([(first, 0.5), (3, 0.25)])
        assert rec["voted_class"] == -1 and rec["vote_weight"] == 0 and not snap["acc"].any() and snap["tracks"]["has_vote"][0] == 0
    # an out-of-range entry at j = 2 is skipped: neither the weight nor an accumulator sees it
    rec, snap = run([(1, 0.5), (3, 0.25), (NC, 0.125), (5, 0.0625)])
    assert rec["vote_weight"] == np.float32(0.8125) and snap["acc"][0].tolist() == [0, 0.5, 0, 0.25, 0, 0.0625, 0, 0, 0, 0]
    # two frames at vote_decay 0.5: acc and wsum decay before the new vote is added
    rec, snap = run([(1, 0.5), (3, 0.25)], frames=2)
    assert snap["acc"][0, 1] == np.float32(0.75) and snap["acc"][0, 3] == np.float32(0.375) and rec["vote_weight"] == np.float32(1.125)
    assert rec["voted_conf"] == np.float32(np.float32(0.75) / np.float32(1.125))


def test_gpu_tracker_scenes_qualify():
    """the scenes tests/test_gpu_topk.py uses keep a decision margin above 1e-4 (as tests/test_gpu_tracking.py demands)"""
    import test_gpu_topk as G
    ok = [s for s in G.SCENE_SEEDS if R.scene_margin(*R.make_scene(s, 16, G.NC_TRACK, n_frames=G.SCENE_FRAMES), 16, G.NC_TRACK, max_tracks=8) > 1e-4]
    assert ok == list(G.SCENE_SEEDS) and len(ok) >= 4
    for i, case in enumerate(G.TRACK_CASES):   # and as they are run there: the records, the decay, the interleaved streams
        *_, ref, want = G.tracker_case(i)
        assert ref.min_margin > G.MARGIN, (case, ref.min_margin)
        assert (want["voted_class"] >= 0).any() and (want["track_id"] > 0).any()
    for seed in (0, 2):   # test_one_entry_records_equal_lp_track_on_the_device's interleaving
        dets, counts = R.make_scene(seed, 16, G.NC_TRACK, n_frames=G.SCENE_FRAMES)
        ref = R.TrackerRef(max_det=16, num_classes=G.NC_TRACK, max_tracks=8, n_streams=3)
        ref.track(dets, counts, G.stream_ids(len(counts), 3))
        assert ref.min_margin > G.MARGIN, (seed, ref.min_margin)


# ---------------------------------------------------------------------------- option errors
def test_pipeline_refuses_distribution_vote_without_track_or_topk():
    from litepi import backend
    for kw in (dict(track_vote="distribution"), dict(track_vote="distribution", track=True), dict(track_vote="distribution", topk=3),
               dict(track_vote="distribution", track=True, topk=0), dict(track_vote="majority", track=True, topk=3), dict(topk=9), dict(topk=-1)):
        with pytest.raises(ValueError) as ei:
            backend.HybridPipeline("no_such.param", "no_such.bin", "no_such.pth", "shufflenetv2", **kw)
        assert "topk" in str(ei.value) or "track_vote" in str(ei.value), kw
        if kw.get("track_vote") == "distribution":
            assert "topk" in str(ei.value) and "track_vote" in str(ei.value), kw


def test_cli_refuses_distribution_vote_without_track_or_topk():
    from litepi import e2e
    base = ["--raw_frames", "f.yuv", "--frame_size", "64x64"]
    for extra in (["--track_vote", "distribution"], ["--track_vote", "distribution", "--track"], ["--track_vote", "distribution", "--topk", "3"]):
        args = e2e.build_parser().parse_args(base + extra)
        with pytest.raises(SystemExit) as ei:
            e2e.check_frame_args(args)
        assert "--topk" in str(ei.value) and "--track_vote" in str(ei.value), extra
        with pytest.raises(SystemExit):
            e2e.run_evaluation(args)
    for bad in ("0", "9"):
        with pytest.raises(SystemExit) as ei:
            e2e.check_frame_args(e2e.build_parser().parse_args(base + ["--topk", bad]))
        assert "--topk" in str(ei.value)
    with pytest.raises(SystemExit):
        e2e.build_parser().parse_args(["--track_vote", "majority"])
    a = e2e.build_parser().parse_args([])
    assert (a.topk, a.track_vote) == (None, "top1")
    a = e2e.build_parser().parse_args(["--topk", "5", "--track_vote", "distribution"])
    assert (a.topk, a.track_vote) == (5, "distribution")


# ---------------------------------------------------------------------------- the shared header under sanitizers
def test_topk_select_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "topk_select_check")
    src = os.path.join(ROOT, "tests", "native", "topk_select_check.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK" and lines[0].startswith("rule ") and lines[1].startswith("keys ")
