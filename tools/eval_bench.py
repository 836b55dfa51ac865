#!/usr/bin/env python3
"""What device-side evaluation costs behind the pipeline.

    python tools/eval_bench.py [--steps 200] [--warmup 20] [--out profiles/eval_bench.json]

One process, the bench's batch (64 x 640^2, fp16) on a max_det 300 handle at conf 0.25 and at conf 0.001.  Ground truth is made
from the batch's own detections, jittered, 10 per frame.  lp_run_batch_device alone and with lp_eval_device behind it
alternate step by step, every step synchronised; medians with p10 / p90.  The evaluator's own time (plan upload, kernel,
head launch) comes from events around lp_eval_device on the handle's stream.  The yardstick is what it replaces: downloading
the records, decoding them into result dicts' fields and evaluate_predictions' per-frame matching (litepi.e2e.match_predictions)
on the host for the same call.  The log is reset in front of every step, outside the timed region, so no step measures a
full log and none pays for the reset.

Seeded synthetic v1 detector whose class bias puts ~8 candidates per frame over conf 0.25 (bench.py's calibration), random
ShuffleNetV2 classifier, noise frames.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "yolo-litepi_amd"))


def _q(t):
    return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(np.percentile(t, 10)), 4),
                p90_ms=round(float(np.percentile(t, 90)), 4), steps=len(t))


def _alternate(fn_a, fn_b, sync, steps, warmup, before=None):
    ta, tb = [], []
    for i in range(warmup + steps):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
            if before is not None:   # outside the timed region, on both sides
                before()
                sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= warmup:
                acc.append((time.perf_counter() - t0) * 1e3)
    return _q(ta), _q(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from litepi import Engine, ncnn_export
    from litepi._ffi import DET_DTYPE
    from litepi.backend import random_shufflenet_state
    from litepi.e2e import match_predictions

    tmp = tempfile.mkdtemp(prefix="eval_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    rng = np.random.default_rng(7)
    B, MD, NC, NGT = 64, 300, 58, 10
    imgs = rng.integers(0, 256, (B, 640, 640, 3), dtype=np.uint8)
    e = Engine(precision="fp16", max_batch=B, max_det=MD, num_classes=NC)
    e.load_detector(p, b)
    s = np.sort(e.detect_raw(imgs[:16])[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    k = 8 * 16
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
    e.load_detector(p, b)
    e.load_classifier(random_shufflenet_state(NC, seed=3))
    st = torch.cuda.Stream()
    e.set_stream(st.cuda_stream)
    dd = torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    d_img = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    e.eval_create(max_gt=16, max_rows=B * MD)
    res = dict(workload=f"64 x 640x640 frames, fp16, synthetic v1 detector + ShuffleNetV2, max_det {MD}, {NGT} ground-truth boxes per frame, 10 thresholds")

    for name, conf in (("conf_0.25", 0.25), ("conf_0.001", 0.001)):
        def pipeline():
            e.run_batch_device(d_img.data_ptr(), B, 640, 640, conf, 0.45, 50, dd.data_ptr(), dc.data_ptr())

        pipeline()
        e.synchronize()
        dets = dd.cpu().numpy().view(DET_DTYPE).reshape(B, MD)
        kept = dc.cpu().numpy()[:B]
        gts = []
        for f in range(B):   # the frame's first detections, jittered; filled up with boxes of their own where it has fewer
            g = []
            for r in dets[f, :min(int(kept[f]), NGT)]:
                j = rng.integers(-3, 4, 4)
                g.append((max(int(r["cls_class"]), 0), int(r["x1"]) + int(j[0]), int(r["y1"]) + int(j[1]), int(r["x2"]) + int(j[2]), int(r["y2"]) + int(j[3])))
            while len(g) < NGT:
                x, y = (int(v) for v in rng.integers(0, 560, 2))
                g.append((int(rng.integers(0, NC)), x, y, x + int(rng.integers(8, 80)), y + int(rng.integers(8, 80))))
            gts.append(g)

        def scored():
            pipeline()
            e.eval_device(dd.data_ptr(), dc.data_ptr(), B, gts)

        t_plain, t_eval = _alternate(pipeline, scored, e.synchronize, a.steps, a.warmup, before=e.eval_reset)
        ev = []
        for _ in range(50):   # the evaluator alone, from events on the handle's stream
            e.eval_reset()
            e.synchronize()
            pipeline()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            e.eval_device(dd.data_ptr(), dc.data_ptr(), B, gts)
            e1.record(st)
            e.synchronize()
            ev.append(e0.elapsed_time(e1))
        got = e.eval_drain()
        th, tm = [], []
        for _ in range(a.host_reps):   # the yardstick: records to the host, the result dicts' fields, the port's matching
            pipeline()
            e.synchronize()
            t0 = time.perf_counter()
            hd = dd.cpu().numpy().view(DET_DTYPE).reshape(B, MD)
            hc = dc.cpu().numpy()[:B]
            preds = []
            for f in range(B):
                u = hd[f, :hc[f]]
                boxes = np.stack([u["x1"], u["y1"], u["x2"], u["y2"]], 1).astype(int).tolist()
                preds.append([{"bbox": tuple(bb), "conf": c, "cls_class": k_} for bb, c, k_ in
                              zip(boxes, u["det_conf"].astype(np.float64).tolist(), u["cls_class"].tolist())])
            t1 = time.perf_counter()
            match_predictions(preds, gts)
            t2 = time.perf_counter()
            th.append((t2 - t0) * 1e3)
            tm.append((t2 - t1) * 1e3)
        res[name] = dict(pipeline=t_plain, pipeline_plus_eval=t_eval, added_ms=round(t_eval["median_ms"] - t_plain["median_ms"], 4),
                         eval_events=_q(ev), host_download_decode_match=_q(th), host_match_only=_q(tm), kept_total=int(kept.sum()),
                         kept_max=int(kept.max()), rows=int(len(got["rows"])), correct_rows=int((got["rows"]["correct"] != 0).sum()))
    e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
