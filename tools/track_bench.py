#!/usr/bin/env python3
"""What device-side tracking costs behind the pipeline.

    python tools/track_bench.py [--steps 200] [--warmup 20] [--out profiles/track_bench.json]

One process, the bench's batch (64 x 640^2, fp16, conf 0.25).  For each of three shapes of the same 64 frames -- 64 streams
x 1 frame, 8 streams x 8 frames, 1 stream x 64 frames -- lp_run_batch_device alone and with lp_track_device behind it
alternate step by step, every step synchronised; medians with p10 / p90.  The tracker launch's own time comes from events
around lp_track_device on the handle's stream.  The yardstick is what the kernel replaces: downloading the records and
walking them with the NumPy loop of tests/tracking_ref.py on the host for the same call.

Seeded synthetic v1 detector whose class bias puts ~8 candidates per frame over conf 0.25 (bench.py's calibration), random
ShuffleNetV2 classifier, noise frames.  The same 64 frames are fed every step: in the 64 x 1 shape every stream re-sees its
frame (all detections match), in the 1 x 64 shape consecutive frames of the stream are unrelated noise (tracks churn).
Prints one JSON line.
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
sys.path.insert(0, os.path.join(_ROOT, "tests"))


def _q(t):
    return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(np.percentile(t, 10)), 4),
                p90_ms=round(float(np.percentile(t, 90)), 4), steps=len(t))


def _alternate(fn_a, fn_b, sync, steps, warmup):
    ta, tb = [], []
    for i in range(warmup + steps):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
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
    import tracking_ref as R
    from litepi import Engine, ncnn_export
    from litepi._ffi import DET_DTYPE
    from litepi.backend import random_shufflenet_state

    tmp = tempfile.mkdtemp(prefix="track_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    rng = np.random.default_rng(7)
    B, MD, NC = 64, 300, 58
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
    dt = torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda")
    d_img = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    cfg = dict(n_streams=B, max_tracks=64)
    shapes = {"64x1": np.arange(B, dtype=np.int32), "8x8": np.repeat(np.arange(8, dtype=np.int32), 8), "1x64": np.zeros(B, np.int32)}
    res = dict(workload="64 x 640x640 frames, fp16, synthetic v1 detector + ShuffleNetV2, conf 0.25, max_det 300, max_tracks 64")

    def pipeline():
        e.run_batch_device(d_img.data_ptr(), B, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())

    for name, sid in shapes.items():
        e.tracker_create(**cfg)

        def tracked():
            pipeline()
            e.track_device(dd.data_ptr(), dc.data_ptr(), B, dt.data_ptr(), sid)

        t_plain, t_trk = _alternate(pipeline, tracked, e.synchronize, a.steps, a.warmup)
        # the tracker launch alone, from events on the handle's stream
        ev = []
        for _ in range(50):
            pipeline()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            e.track_device(dd.data_ptr(), dc.data_ptr(), B, dt.data_ptr(), sid)
            e1.record(st)
            e.synchronize()
            ev.append(e0.elapsed_time(e1))
        kept = dc.cpu().numpy()[:B]
        # the yardstick: records to the host + the NumPy loop, same call
        ref = R.TrackerRef(max_det=MD, num_classes=NC, **cfg)
        th = []
        for _ in range(a.host_reps):
            pipeline()
            e.synchronize()
            t0 = time.perf_counter()
            dets = dd.cpu().numpy().view(DET_DTYPE).reshape(B, MD)
            counts = dc.cpu().numpy()[:B]
            ref.track(dets, counts, sid)
            th.append((time.perf_counter() - t0) * 1e3)
        res[name] = dict(pipeline=t_plain, pipeline_plus_tracker=t_trk, added_ms=round(t_trk["median_ms"] - t_plain["median_ms"], 4),
                         tracker_events=_q(ev), host_download_plus_numpy=_q(th), kept_total=int(kept.sum()), kept_max=int(kept.max()))
    e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
