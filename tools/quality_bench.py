#!/usr/bin/env python3
"""What crop quality per detection costs.

    python tools/quality_bench.py [--steps 200] [--warmup 20] [--repeats 3] [--baseline-tree DIR] [--out profiles/quality_bench.json]

The bench's batch (64 x 640^2, fp16, conf 0.25, the bench's synthetic weights) through lp_run_batch_device, in child
processes of their own under a time limit (a child that fails or runs out of time ends the run), `repeats` times each, in
turn: the baseline tree's library (a checkout of the parent commit, built; quality does not exist there), this tree with
quality off, this tree with quality on.  Per child:

pipelined  the steps enqueued back to back, synchronised every 20: wall time per step (what bench.py's throughput sees)
synced     every step synchronised: median with p10 / p90
launches   (on only) the eager time of quality_clear and quality_measure from the handle's profiler (lp_profile_next), and
           the measure's achieved bytes per second over R x 3 S^2 crop bytes

The off state is to be compared with the baseline and nothing else: its difference from the baseline's median should lie
inside the spread (max - min over the repeats) of the baseline's own runs; both spreads are recorded.

Seeded synthetic v1 detector whose class bias puts ~8 candidates per frame over conf 0.25 (bench.py's calibration), random
ShuffleNetV2 classifier, noise frames, as tools/topk_bench.py.  Prints one JSON line.
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

B, MD, NC, S = 64, 300, 58, 64
CHUNK = 20


def _q(t):
    return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(np.percentile(t, 10)), 4),
                p90_ms=round(float(np.percentile(t, 90)), 4), steps=len(t))


def _models():
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    tmp = tempfile.mkdtemp(prefix="quality_bench_")
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


def child(a):
    sys.path.insert(0, os.path.join(os.path.abspath(a.tree), "yolo-litepi_amd"))
    import torch
    from litepi import Engine
    p, b, sd, imgs = _models()
    d_img = torch.from_numpy(imgs).cuda()
    dd = torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e = Engine(precision="fp16", max_batch=B, max_det=MD, num_classes=NC)
    e.load_detector(p, b)
    e.load_classifier(sd)
    if a.mode == "on":
        e.quality_enable(True)

    def step():
        e.run_batch_device(d_img.data_ptr(), B, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
    for _ in range(a.warmup):
        step()
    e.synchronize()
    piped = []
    for _ in range(max(a.steps // CHUNK, 1)):
        t0 = time.perf_counter()
        for _ in range(CHUNK):
            step()
        e.synchronize()
        piped.append((time.perf_counter() - t0) * 1e3 / CHUNK)
    synced = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        step()
        e.synchronize()
        synced.append((time.perf_counter() - t0) * 1e3)
    res = {"mode": a.mode, "pipelined": _q(piped), "synced": _q(synced), "kept_total": int(dc.cpu().numpy()[:B].sum())}
    per = {}
    for _ in range(7):   # the profiled step is eager; the launches' own time from the events around each
        e.profile_next(True)
        step()
        e.synchronize()
        for r in e.profile_read():
            if r["layer"] == "quality":
                per.setdefault(r["name"], []).append(r["ms"])
    if a.mode == "on":
        rois = e.roi_overflow()[0]
        res["launches_us"] = {n: round(float(np.median(v)) * 1e3, 2) for n, v in per.items()}
        res["rois"] = rois
        res["crop_bytes"] = rois * 3 * S * S
        res["measure_gb_per_s"] = round(rois * 3 * S * S / (float(np.median(per["quality_measure"])) * 1e-3) / 1e9, 2)
    else:
        assert not per, "quality off must add no launch"
    e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-tree", type=str, default=None, help="a built checkout of the parent commit; absent: no baseline is measured")
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--mode", choices=["off", "on"], default=None, help="run one measurement in this process (what the parent process starts)")
    ap.add_argument("--tree", type=str, default=_ROOT, help="with --mode: the tree whose library is measured")
    ap.add_argument("--child-timeout", type=int, default=180, help="seconds a child may take")
    a = ap.parse_args()
    if a.mode:
        print(json.dumps(child(a)))
        return 0
    plan = ([("baseline_off", a.baseline_tree, "off")] if a.baseline_tree else []) + [("off", _ROOT, "off"), ("on", _ROOT, "on")]
    runs = {name: [] for name, _, _ in plan}
    for _ in range(a.repeats):
        for name, tree, mode in plan:
            cmd = [sys.executable, os.path.abspath(__file__), "--mode", mode, "--tree", tree, "--steps", str(a.steps), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
            except subprocess.TimeoutExpired:
                print(f"quality_bench: {name} ran longer than {a.child_timeout} s; nothing more is started", file=sys.stderr)
                return 1
            if r.returncode != 0:
                print(f"quality_bench: {name} ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = {"workload": "64 x 640x640 frames, fp16, synthetic v1 detector + ShuffleNetV2 (58 classes), conf 0.25, max_det 300, cls_input 64",
           "runs": runs, "summary": {}}
    for name, rs in runs.items():
        for kind in ("pipelined", "synced"):
            m = [r[kind]["median_ms"] for r in rs]
            res["summary"][f"{name}_{kind}"] = dict(median_of_medians_ms=round(float(np.median(m)), 4), spread_ms=round(max(m) - min(m), 4), medians_ms=m)
    sm = res["summary"]
    if "baseline_off_pipelined" in sm:
        for kind in ("pipelined", "synced"):
            diff = sm[f"off_{kind}"]["median_of_medians_ms"] - sm[f"baseline_off_{kind}"]["median_of_medians_ms"]
            sm[f"off_minus_baseline_{kind}_ms"] = round(diff, 4)
            sm[f"off_within_baseline_spread_{kind}"] = bool(abs(diff) <= sm[f"baseline_off_{kind}"]["spread_ms"])
    for kind in ("pipelined", "synced"):
        sm[f"on_minus_off_{kind}_ms"] = round(sm[f"on_{kind}"]["median_of_medians_ms"] - sm[f"off_{kind}"]["median_of_medians_ms"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
