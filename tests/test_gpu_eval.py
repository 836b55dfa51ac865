"""Device-side evaluation on the GPU: the kernel against the rule (tests/eval_ref.py) bit for bit, row order across calls and
a wrapping ring, the full log, errors, no effect on other paths, and the evaluator behind the pipeline, HybridPipeline and the
CLI."""
import json
import os

import numpy as np
import pytest
import torch

import eval_ref as R

pytestmark = pytest.mark.gpu

NC = 6
MAX_BATCH = 12
UNSORTED16 = np.array([0.2 + 0.05 * ((j * 7) % 16) for j in range(16)])
THRS = {1: np.array([0.5]), 10: R.THR10, 16: UNSORTED16}


@pytest.fixture(scope="module")
def engines():
    from litepi import Engine
    es = {md: Engine(precision="fp16", max_batch=MAX_BATCH, max_det=md, num_classes=NC) for md in (16, 300, 1100)}
    yield es
    for e in es.values():
        e.close()


def pack(frames, max_det, counts=None):
    """[(dets, gts)] -> ([B, max_det] records, [B] int32 counts, [gts])"""
    from litepi._ffi import DET_DTYPE
    d = np.zeros((len(frames), max_det), dtype=DET_DTYPE)
    for b, (f, _) in enumerate(frames):
        d[b, :len(f)] = f
    c = np.array([len(f) for f, _ in frames], dtype=np.int32) if counts is None else np.asarray(counts, dtype=np.int32)
    return d, c, [g for _, g in frames]


def upload(d, c):
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(d.view(np.uint8).reshape(-1).copy()).to(dev), torch.from_numpy(np.concatenate([c, np.zeros(2 * len(c), np.int32)])).to(dev))


def assert_matches(got, frames, thr, tag):
    for b, (dets, gts) in enumerate(frames):
        want = R.match(dets, gts, thr)
        assert got[b, :len(dets)].tobytes() == want.tobytes(), f"{tag}: frame {b} ({len(dets)} records, {len(gts)} boxes)"
        assert not got[b, len(dets):].view(np.uint8).any(), f"{tag}: frame {b} wrote beyond its count"


def assert_drain(eng, frames, thr, tag, first_frame=0, dropped=0):
    got = eng.eval_drain()
    rows, _ = R.rows_of(frames, thr, first_frame)
    assert got["rows"].tobytes() == rows.tobytes(), f"{tag}: rows"
    assert got["gt_per_class"].tolist() == R.gt_per_class(frames, NC).tolist(), f"{tag}: class counts"
    assert (got["frames"], got["dropped"]) == (first_frame + len(frames), dropped), tag
    return got


# ---------------------------------------------------------------------------- 1. the kernel equals the rule
@pytest.mark.parametrize("n_thr", [1, 10, 16])
@pytest.mark.parametrize("md", [16, 300, 1100])
def test_kernel_equals_the_rule(engines, md, n_thr):
    from litepi._ffi import MATCH_DTYPE
    eng, thr, max_gt = engines[md], THRS[n_thr], 128
    eng.eval_create(max_gt=max_gt, thr=thr, max_rows=MAX_BATCH * md)
    rng = np.random.default_rng(100 * md + n_thr)
    Ps = [p for p in (0, 1, 63, 64, 65, md) if p <= md]
    Gs = (0, 1, 64, 65, max_gt)
    k = 0
    for B in (1, 3, MAX_BATCH):
        frames = []
        for b in range(B):
            P, G = Ps[(k + b) % len(Ps)], Gs[(k // 2 + b) % len(Gs)]
            frames.append(R.scene(rng, P, G, NC, W=2048 if G < 64 else 700))
        k += B + 1
        d, c, gts = pack(frames, md)
        tag = f"max_det {md} n_thr {n_thr} B {B}"
        eng.eval_reset()
        assert_matches(eng.evaluate(d, c, gts), frames, thr, tag + " host records")
        assert_drain(eng, frames, thr, tag + " host records")
        eng.eval_reset()
        dd, dc = upload(d, c)
        dm = torch.zeros(B * md * 16, dtype=torch.uint8, device=dd.device)
        eng.eval_device(dd.data_ptr(), dc.data_ptr(), B, gts, dm.data_ptr())
        eng.synchronize()
        assert_matches(dm.cpu().numpy().view(MATCH_DTYPE).reshape(B, md), frames, thr, tag + " device records")
        assert_drain(eng, frames, thr, tag + " device records")
        eng.eval_reset()
        eng.eval_device(dd.data_ptr(), dc.data_ptr(), B, gts)   # without lp_match records
        assert_drain(eng, frames, thr, tag + " no match records")


@pytest.mark.parametrize("md", [16, 300, 1100])
def test_full_ground_truth_table(engines, md):
    """G = max_gt = 256 (the whole LDS table) with P = max_det and 16 unsorted thresholds in one frame, beside an empty frame"""
    from litepi._ffi import MATCH_DTYPE
    eng = engines[md]
    eng.eval_create(max_gt=256, thr=UNSORTED16, max_rows=3 * md)
    rng = np.random.default_rng(256 + md)
    frames = [R.scene(rng, md, 256, NC, W=700), R.scene(rng, 0, 256, NC, W=700), R.scene(rng, md, 255, NC, W=500)]
    d, c, gts = pack(frames, md)
    assert_matches(eng.evaluate(d, c, gts), frames, UNSORTED16, f"max_det {md} G 256 host records")
    assert_drain(eng, frames, UNSORTED16, f"max_det {md} G 256 host records")
    eng.eval_reset()
    dd, dc = upload(d, c)
    dm = torch.zeros(3 * md * 16, dtype=torch.uint8, device=dd.device)
    eng.eval_device(dd.data_ptr(), dc.data_ptr(), 3, gts, dm.data_ptr())
    eng.synchronize()
    assert_matches(dm.cpu().numpy().view(MATCH_DTYPE).reshape(3, md), frames, UNSORTED16, f"max_det {md} G 256 device records")
    assert_drain(eng, frames, UNSORTED16, f"max_det {md} G 256 device records")


def test_kept_counts_are_clamped(engines):
    eng, md = engines[16], 16
    eng.eval_create(max_gt=8)
    rng = np.random.default_rng(5)
    full = [R.scene(rng, md, 5, NC) for _ in range(3)]
    d, _, gts = pack(full, md)
    counts = [-3, md + 5, 7]
    frames = [(full[0][0][:0], gts[0]), (full[1][0], gts[1]), (full[2][0][:7], gts[2])]
    assert_matches(eng.evaluate(d, counts, gts), frames, R.THR10, "clamped")
    assert_drain(eng, frames, R.THR10, "clamped")


@pytest.mark.parametrize("md", [16, 1100])
def test_hand_built_frames(engines, md):
    eng = engines[md]
    hand = R.hand_frames()
    for thr_key in {tuple(v[2]) for v in hand.values()}:
        names = sorted(n for n, v in hand.items() if tuple(v[2]) == thr_key)
        thr = np.array(thr_key)
        eng.eval_create(max_gt=4, thr=thr)
        frames = [(hand[n][0], hand[n][1]) for n in names]
        d, c, gts = pack(frames, md)
        got = eng.evaluate(d, c, gts)
        assert_matches(got, frames, thr, f"hand-built {names}")
        for b, n in enumerate(names):
            for p, (bits, gt) in hand[n][3].items():
                assert (int(got[b, p]["correct"]), int(got[b, p]["gt"])) == (bits, gt), (n, p)
        assert_drain(eng, frames, thr, f"hand-built {names}")


# ---------------------------------------------------------------------------- 2. order and splitting
def test_rows_do_not_depend_on_the_split_and_the_ring_wraps(engines):
    eng, md = engines[300], 300
    rng = np.random.default_rng(9)
    frames = [R.scene(rng, int(rng.integers(0, 120)), int(rng.integers(0, 12)), NC) for _ in range(12)]
    d, c, gts = pack(frames, md)
    drained = []
    for chunk in (12, 4, 1):
        eng.eval_create(max_gt=16)
        bufs = [upload(d[i:i + chunk], c[i:i + chunk]) for i in range(0, 12, chunk)]
        torch.cuda.synchronize()
        for k, (dd, dc) in enumerate(bufs):   # no synchronise in between
            eng.eval_device(dd.data_ptr(), dc.data_ptr(), chunk, gts[k * chunk:(k + 1) * chunk])
        got = assert_drain(eng, frames, R.THR10, f"{12 // chunk} calls of {chunk}")
        assert got["rows"]["frame"].tolist() == np.repeat(np.arange(12), c).tolist()
        drained.append((got["rows"].tobytes(), got["gt_per_class"].tobytes(), got["frames"]))
    assert drained[0] == drained[1] == drained[2]
    assert drained[0][2] == 12
    # twenty calls back to back on a ring of 8 slots, each with other ground truth: a slot re-used too early would show
    eng.eval_create(max_gt=16)
    seq = [frames[k % 12] for k in range(20)]
    bufs = [upload(*pack([f], md)[:2]) for f in seq]
    torch.cuda.synchronize()
    for (dd, dc), f in zip(bufs, seq):
        eng.eval_device(dd.data_ptr(), dc.data_ptr(), 1, [f[1]])
    assert_drain(eng, seq, R.THR10, "20 calls on 8 slots")


# ---------------------------------------------------------------------------- 3. a full log
def test_log_overflow_and_reset(engines):
    eng, md = engines[300], 300
    rng = np.random.default_rng(10)
    frames = [R.scene(rng, 40 + 3 * k, 6, NC) for k in range(6)]
    total = sum(len(f) for f, _ in frames)
    cap = 40 + 43 + 20   # the log ends inside the third frame
    eng.eval_create(max_gt=8, max_rows=cap)
    d, c, gts = pack(frames, md)
    eng.evaluate(d[:3], c[:3], gts[:3])
    eng.evaluate(d[3:], c[3:], gts[3:])   # the head is past the log: nothing is written
    want, _ = R.rows_of(frames)
    got = eng.eval_drain()
    assert len(got["rows"]) == cap and got["rows"].tobytes() == want[:cap].tobytes()
    assert (got["dropped"], got["frames"]) == (total - cap, 6)
    assert got["gt_per_class"].tolist() == R.gt_per_class(frames, NC).tolist()
    eng.eval_reset()
    empty = eng.eval_drain()
    assert (len(empty["rows"]), empty["dropped"], empty["frames"], int(empty["gt_per_class"].sum())) == (0, 0, 0, 0)
    eng.evaluate(d[:2], c[:2], gts[:2])
    assert_drain(eng, frames[:2], R.THR10, "after reset")


# ---------------------------------------------------------------------------- 4. errors
def test_errors_leave_the_handle_usable():
    from litepi import Engine, _ffi
    eng = Engine(precision="fp16", max_batch=4, max_det=16, num_classes=NC)
    try:
        rng = np.random.default_rng(12)
        frames = [R.scene(rng, 10, 3, NC) for _ in range(4)]
        d, c, gts = pack(frames, 16)
        dd, dc = upload(d, c)

        def code(fn):
            with pytest.raises(_ffi.LitepiError) as ei:
                fn()
            return ei.value.code

        assert code(lambda: eng.evaluate(d, c, gts)) == _ffi.LP_ERR_STATE
        assert code(lambda: eng.eval_device(dd.data_ptr(), dc.data_ptr(), 4, gts)) == _ffi.LP_ERR_STATE
        assert code(eng.eval_drain) == _ffi.LP_ERR_STATE and code(eng.eval_reset) == _ffi.LP_ERR_STATE
        eng.eval_destroy()   # without an evaluator: nothing to do
        assert code(lambda: eng.eval_create(max_gt=0)) == _ffi.LP_ERR_ARG
        eng.eval_create(max_gt=3)
        for B in (0, -1, 5):
            assert code(lambda: eng.eval_device(dd.data_ptr(), dc.data_ptr(), B, gts[:max(B, 0)] if B < 5 else gts + gts[:1])) == _ffi.LP_ERR_ARG
        too_many = gts[:3] + [gts[3] + gts[3][:1]]   # four boxes, max_gt = 3
        assert code(lambda: eng.evaluate(d, c, too_many)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.eval_device(dd.data_ptr(), dc.data_ptr(), 4, too_many)) == _ffi.LP_ERR_ARG
        for bad_cls in (-1, NC):
            bad = gts[:3] + [[(bad_cls,) + gts[3][0][1:]] + gts[3][1:]]
            assert code(lambda: eng.evaluate(d, c, bad)) == _ffi.LP_ERR_ARG
            assert code(lambda: eng.eval_device(dd.data_ptr(), dc.data_ptr(), 4, bad)) == _ffi.LP_ERR_ARG
        assert code(lambda: eng.eval_device(dd.data_ptr() + 8, dc.data_ptr(), 4, gts)) == _ffi.LP_ERR_ARG
        dm = torch.zeros(4 * 16 * 16 + 16, dtype=torch.uint8, device=dd.device)
        assert code(lambda: eng.eval_device(dd.data_ptr(), dc.data_ptr(), 4, gts, dm.data_ptr() + 4)) == _ffi.LP_ERR_ARG
        n = _ffi.C.c_int()
        rows = np.zeros(1, dtype=_ffi.EVAL_ROW_DTYPE)
        eng.evaluate(d, c, gts)
        assert eng.lib.lp_eval_drain(eng._h, rows.ctypes.data, 1, _ffi.C.byref(n), None, None, None) == _ffi.LP_ERR_ARG and n.value == 40
        # none of the refused calls left a trace: the log holds the one good call, and another gives the right result
        assert_drain(eng, frames, R.THR10, "after the errors")
        assert_matches(eng.evaluate(d, c, gts), frames, R.THR10, "after the errors")
        assert_drain(eng, frames + frames, R.THR10, "after the errors, second call")
        eng.eval_destroy()
        assert code(eng.eval_drain) == _ffi.LP_ERR_STATE
    finally:
        eng.close()


# ---------------------------------------------------------------------------- models for 5 and 6
PH, PW = 240, 320


@pytest.fixture(scope="module")
def cls_state():
    from litepi.backend import random_shufflenet_state
    return random_shufflenet_state(91, seed=3)


def model_engine(synth_models, cls_state, max_batch=8, max_det=32):
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=max_batch, max_det=max_det, num_classes=91)
    e.load_detector(*synth_models["v1"])
    e.load_classifier(cls_state)
    return e


def clip_frames(seed, n=8, H=PH, W=PW):
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (40, 40, 3), dtype=np.uint8)
    for k in range(n):
        f[k, 100:140, 80 + 4 * k:120 + 4 * k] = patch
    return f


def jittered_gts(dets, counts, seed, max_gt):
    """ground truth from a pass's boxes: integer boxes moved by up to 2 pixels, the record's class (or 0 when unclassified)"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(len(counts)):
        d = dets[b, :min(int(counts[b]), max_gt)]
        box = R.det_boxes(d) + rng.integers(-2, 3, (len(d), 4))
        out.append([(max(int(k), 0), *(int(v) for v in bb)) for k, bb in zip(d["cls_class"], box)])
    return out


# ---------------------------------------------------------------------------- 5. no side effect
def test_unused_evaluator_changes_nothing(synth_models, cls_state):
    x_host = clip_frames(3, n=4)
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(x_host).to(dev)
    B = len(x_host)
    results = []
    for state in ("none", "unused", "destroyed"):
        eng = model_engine(synth_models, cls_state)
        try:
            if state != "none":
                eng.eval_create(max_gt=16)
            if state == "destroyed":
                eng.eval_destroy()
            d = torch.zeros(B * 32 * 32, dtype=torch.uint8, device=dev)
            c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
            outs = []
            for call in range(3):   # eager, capture, replay
                eng.run_batch_device(x.data_ptr(), B, PH, PW, 0.05, 0.45, 50, d.data_ptr(), c.data_ptr())
                eng.synchronize()
                outs.append((d.cpu().numpy().tobytes(), c.cpu().numpy().tobytes()))
            eng.profile_next(True)
            eng.run_batch_device(x.data_ptr(), B, PH, PW, 0.05, 0.45, 50, d.data_ptr(), c.data_ptr())
            eng.synchronize()
            results.append((outs, [(r["name"], r["layer"]) for r in eng.profile_read()]))
        finally:
            eng.close()
    for k, state in ((1, "unused"), (2, "destroyed")):
        assert results[0][0] == results[k][0], f"lp_run_batch_device output differs on a handle with an evaluator ({state})"
        assert results[0][1] == results[k][1] and len(results[0][1]) > 10, f"the launch list differs on a handle with an evaluator ({state})"
    assert not any("eval" in name for name, _ in results[1][1])


# ---------------------------------------------------------------------------- 6. behind the pipeline
# (0.5, 0.25): the thresholds of a labelled run; (0.05, 0.04): where the synthetic detector's scores lie, so that records exist
CONF_PAIRS = [(0.5, 0.25), (0.05, 0.04)]


def metrics_pair(rows, frames, nc):
    from litepi.e2e import metrics_from_rows
    want_rows, _ = R.rows_of(frames)
    assert rows.tobytes() == want_rows.tobytes()
    per = R.gt_per_class(frames, nc)
    return metrics_from_rows(rows, per, nc, 10), metrics_from_rows(want_rows, per, nc, 10)


def same_metrics(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k


def port_metrics(frames, nc):
    from litepi.e2e import evaluate_predictions
    return evaluate_predictions([R.result_dicts(d) for d, _ in frames], [g for _, g in frames], nc)


@pytest.mark.parametrize("gt_conf,conf", CONF_PAIRS)
def test_eval_device_behind_run_batch_device(synth_models, cls_state, gt_conf, conf):
    from litepi._ffi import DET_DTYPE
    x_host = clip_frames(21)
    B, md, max_gt = len(x_host), 32, 32
    dev = torch.device("cuda", 0)
    eng = model_engine(synth_models, cls_state)
    try:
        d0, c0, _, _ = eng.run_batch(list(x_host), gt_conf, 0.45, 50)
        gts = jittered_gts(d0, c0, 77, max_gt)
        eng.eval_create(max_gt=max_gt)
        x = torch.from_numpy(x_host).to(dev)
        d = torch.zeros(B * md * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        eng.run_batch_device(x.data_ptr(), B, PH, PW, conf, 0.45, 50, d.data_ptr(), c.data_ptr())
        eng.eval_device(d.data_ptr(), c.data_ptr(), B, gts)   # no synchronise in between
        got = eng.eval_drain()
        dets, counts = d.cpu().numpy().view(DET_DTYPE).reshape(B, md), c.cpu().numpy()[:B]
        frames = [(dets[b, :counts[b]], gts[b]) for b in range(B)]
        m, want = metrics_pair(got["rows"], frames, 91)
        same_metrics(m, want)
        assert got["gt_per_class"].tolist() == R.gt_per_class(frames, 91).tolist() and got["frames"] == B
        assert sum(R.ties(f, g) for f, g in frames) == 0, "the fixed seeds give a tie-free run: the port is defined on it"
        same_metrics(m, port_metrics(frames, 91))
        if conf < 0.25:   # the pair chosen for the synthetic detector: the run is not empty
            assert len(got["rows"]) >= B and sum(len(g) for g in gts) >= B and got["rows"]["correct"].any()
    finally:
        eng.close()


@pytest.mark.parametrize("mode", ["plain", "tiled"])
@pytest.mark.parametrize("gt_conf,conf", CONF_PAIRS)
def test_hybrid_pipeline_evaluate(synth_models, cls_state, tmp_path, mode, gt_conf, conf):
    from litepi import HybridPipeline
    p, b = synth_models["v1"]
    cls_file = str(tmp_path / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in cls_state.items()}, cls_file)
    kw = dict(num_classes=91, precision="fp16", max_batch=8, max_det=32)
    imgs = list(clip_frames(31))
    if mode == "tiled":
        kw.update(tile_overlap=128, max_batch=16)
        imgs = list(clip_frames(32, n=4, H=800, W=1000))
    pipe = HybridPipeline(p, b, cls_file, "shufflenetv2", evaluate=dict(max_gt=32), **kw)
    try:
        first = pipe.run_batch(imgs, gt_conf, 0.45, 50, evaluate=False)
        assert pipe.engine.eval_drain()["frames"] == 0, "evaluate=False must not feed the evaluator"
        rng = np.random.default_rng(5)
        gts = [[(max(r["cls_class"], 0), *(int(v) + int(rng.integers(-2, 3)) for v in r["bbox"])) for r in res[:32]] for res, _ in first]
        got = pipe.run_batch(imgs, conf, 0.45, 50, gts=gts)
        m = pipe.evaluation()
        frames = [(R.make_dets([r["bbox"] for r in res], [r["det_conf"] for r in res], [r["cls_class"] for r in res]), g)
                  for (res, _), g in zip(got, gts)]
        rows, _ = R.rows_of(frames)
        from litepi.e2e import metrics_from_rows
        same_metrics(m, metrics_from_rows(rows, R.gt_per_class(frames, 91), 91, 10))
        assert (pipe.eval_frames, pipe.eval_rows_dropped) == (len(imgs), 0)
        assert sum(R.ties(f, g) for f, g in frames) == 0, "the fixed seeds give a tie-free run: the port is defined on it"
        same_metrics(m, port_metrics(frames, 91))
        if conf < 0.25:
            assert len(rows) >= len(imgs) and rows["correct"].any()
        with pytest.raises(ValueError, match="gts"):
            pipe.run_batch(imgs, conf, 0.45, 50)
    finally:
        pipe.close()


def test_e2e_device_eval_equals_the_host_evaluator(synth_models, cls_state, tmp_path, capsys):
    from litepi import e2e
    from litepi.e2e import metrics_from_rows
    p, b = synth_models["v1"]
    cls_file = str(tmp_path / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in cls_state.items()}, cls_file)
    clip = clip_frames(41, n=7)
    clip.tofile(tmp_path / "clip.bgr")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(91)}))
    labels = tmp_path / "labels"
    labels.mkdir()
    base = ["--detector_param", p, "--detector_bin", b, "--classifier", cls_file, "--clf_arch", "shufflenetv2", "--labels", str(labels),
            "--classes", str(classes), "--batch_images", "3", "--max_det", "32", "--raw_frames", str(tmp_path / "clip.bgr"), "--frame_size",
            f"{PW}x{PH}", "--benchmark_conf", "0.25", "--yolo_conf", "0.04", "--warmup", "1"]
    # labels from a first run's detections: YOLO text (class, centre and size, normalised), two thirds of every frame's boxes
    r0 = e2e.run_evaluation(e2e.build_parser().parse_args(base + ["--output", str(tmp_path / "out0")]))
    for k, preds in enumerate(r0["all_preds"]):
        lines = []
        for q in preds[:max(1, 2 * len(preds) // 3)][:16]:
            x1, y1, x2, y2 = q["bbox"]
            lines.append(f"{max(q['cls_class'], 0)} {(x1 + x2) / 2 / PW:.6f} {(y1 + y2) / 2 / PH:.6f} {(x2 - x1) / PW:.6f} {(y2 - y1) / PH:.6f}\n")
        (labels / f"frame_{k + 1:06d}.txt").write_text("".join(lines))
    host = e2e.run_evaluation(e2e.build_parser().parse_args(base + ["--output", str(tmp_path / "out1")]))
    dev = e2e.run_evaluation(e2e.build_parser().parse_args(base + ["--output", str(tmp_path / "out2"), "--device_eval", "--device_eval_max_gt", "16"]))
    capsys.readouterr()
    assert host["all_gts"] == dev["all_gts"] and host["all_preds"] == dev["all_preds"] and sum(len(g) for g in host["all_gts"]) >= 7
    frames = [(R.make_dets([q["bbox"] for q in pr], [q["conf"] for q in pr], [q["cls_class"] for q in pr]), g)
              for pr, g in zip(dev["all_preds"], dev["all_gts"])]
    rows, _ = R.rows_of(frames)
    same_metrics(dev["metrics"], metrics_from_rows(rows, R.gt_per_class(frames, 91), 91, 10))
    assert sum(R.ties(f, g) for f, g in frames) == 0, "the fixed seed gives a tie-free run: the port is defined on it"
    same_metrics(dev["metrics"], host["metrics"])
    with pytest.raises(SystemExit, match="more than --device_eval_max_gt 1"):
        e2e.run_evaluation(e2e.build_parser().parse_args(base + ["--output", str(tmp_path / "out3"), "--device_eval", "--device_eval_max_gt", "1"]))
    capsys.readouterr()
