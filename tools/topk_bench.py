#!/usr/bin/env python3
"""What top-k per detection and the distribution vote cost.

    python tools/topk_bench.py [--steps 200] [--warmup 20] [--out profiles/topk_bench.json]

Two parts, each a child process of its own under a time limit (a part that fails or runs out of time ends the run):

pipeline  the bench's batch (64 x 640^2, fp16, conf 0.25, the bench's synthetic weights): lp_run_batch_device on four handles
          that differ in lp_topk_enable only -- off, k = 1, 5, 8 -- alternating step by step, every step synchronised;
          medians with p10 / p90.  The two launches' own time comes from the handle's profiler (lp_profile_next), one
          eager step per handle: the clear is a launch of its own in front of the select.
tracker   events around lp_track_device and lp_track_topk_device on the handle's stream behind the same pipeline step
          (k = 5), alternating call by call on one tracker, for three shapes of the same 64 frames: 64 streams x 1 frame,
          8 x 8, 1 x 64.

Seeded synthetic v1 detector whose class bias puts ~8 candidates per frame over conf 0.25 (bench.py's calibration), random
ShuffleNetV2 classifier, noise frames, as tools/inventory_bench.py.  Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "yolo-litepi_amd"))

B, MD, NC = 64, 300, 58
KS = (0, 1, 5, 8)


def _q(t):
    return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(np.percentile(t, 10)), 4),
                p90_ms=round(float(np.percentile(t, 90)), 4), steps=len(t))


def _models():
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    tmp = tempfile.mkdtemp(prefix="topk_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    imgs = np.random.default_rng(7).integers(0, 256, (B, 640, 640, 3), dtype=np.uint8)
    e = Engine(precision="fp16", max_batch=B, max_det=MD, num_classes=NC)
    e.load_detector(p, b)
    s = np.sort(e.detect_raw(imgs[:16])[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    e.close()
    k = 8 * 16
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
    return p, b, random_shufflenet_state(NC, seed=3), imgs


def _engine(p, b, sd, k):
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=B, max_det=MD, num_classes=NC)
    e.load_detector(p, b)
    e.load_classifier(sd)
    e.topk_enable(k)
    return e


def part_pipeline(a):
    import torch
    p, b, sd, imgs = _models()
    d_img = torch.from_numpy(imgs).cuda()
    dd = torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    engines = {k: _engine(p, b, sd, k) for k in KS}
    times = {k: [] for k in KS}
    for i in range(a.warmup + a.steps):
        for k in KS:
            e = engines[k]
            t0 = time.perf_counter()
            e.run_batch_device(d_img.data_ptr(), B, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            if i >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    res = {"workload": "64 x 640x640 frames, fp16, synthetic v1 detector + ShuffleNetV2 (58 classes), conf 0.25, max_det 300",
           "kept_total": int(dc.cpu().numpy()[:B].sum()), "step": {}, "launches": {}}
    for k in KS:
        res["step"]["off" if k == 0 else f"k{k}"] = _q(times[k])
        e = engines[k]
        per = {}
        for _ in range(5):   # the profiled step is eager; the launches' own time from the events around each
            e.profile_next(True)
            e.run_batch_device(d_img.data_ptr(), B, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            for r in e.profile_read():
                if r["name"].startswith("topk"):
                    per.setdefault(r["name"], []).append(r["ms"])
        if k:
            res["launches"][f"k{k}"] = {n: round(float(np.median(v)) * 1e3, 2) for n, v in per.items()}   # microseconds
        else:
            assert not per, "top-k off must add no launch"
        e.close()
    off = res["step"]["off"]["median_ms"]
    res["added_ms"] = {n: round(v["median_ms"] - off, 4) for n, v in res["step"].items() if n != "off"}
    res["clear_is_a_launch_of_its_own"] = True
    return res


def part_tracker(a):
    import torch
    p, b, sd, imgs = _models()
    e = _engine(p, b, sd, 5)
    st = torch.cuda.Stream()
    e.set_stream(st.cuda_stream)
    d_img = torch.from_numpy(imgs).cuda()
    dd = torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    dt = torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    addr, _ = e.topk_buffer()
    shapes = {"64x1": np.arange(B, dtype=np.int32), "8x8": np.repeat(np.arange(8, dtype=np.int32), 8), "1x64": np.zeros(B, np.int32)}
    res = {}
    for name, sid in shapes.items():
        e.tracker_create(n_streams=B, max_tracks=64)
        ev = {"lp_track_device": [], "lp_track_topk_device": []}
        for i in range(a.warmup + a.steps):
            for call in ev:
                e.run_batch_device(d_img.data_ptr(), B, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                if call == "lp_track_device":
                    e.track_device(dd.data_ptr(), dc.data_ptr(), B, dt.data_ptr(), sid)
                else:
                    e.track_topk_device(dd.data_ptr(), dc.data_ptr(), addr, B, dt.data_ptr(), sid)
                e1.record(st)
                e.synchronize()
                if i >= a.warmup:
                    ev[call].append(e0.elapsed_time(e1))
        res[name] = {c: _q(t) for c, t in ev.items()}
        res[name]["added_ms"] = round(res[name]["lp_track_topk_device"]["median_ms"] - res[name]["lp_track_device"]["median_ms"], 4)
    res["kept_total"] = int(dc.cpu().numpy()[:B].sum())
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--part", choices=["pipeline", "tracker"], default=None, help="run one part in this process (what the parent starts)")
    ap.add_argument("--part-timeout", type=int, default=240, help="seconds a part may take")
    a = ap.parse_args()
    if a.part:
        print(json.dumps({"pipeline": part_pipeline, "tracker": part_tracker}[a.part](a)))
        return 0
    res = {}
    for part in ("pipeline", "tracker"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=a.part_timeout)
        except subprocess.TimeoutExpired:
            print(f"topk_bench: part {part} ran longer than {a.part_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if r.returncode != 0:
            print(f"topk_bench: part {part} ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res[part] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
