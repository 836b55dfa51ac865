#!/usr/bin/env python3
"""Rectangular detector input: frames/s of 1080p video on a square and on two rectangular handles.

    python tools/rect_bench.py [--frames 64] [--steps 30] [--warmup 8] [--rounds 3] [--out profiles/rect_bench.json]

`frames` device-resident 1080 x 1920 BGR frames per call through lp_run_batch_device (letterbox, detector, NMS, ROI resize,
classifier; the captured step replays), fp16, handles of capacity `frames` with det_input 640 x 640, 384 x 640 and 320 x 640,
seeded v1 and v2 detectors (one seed = the same weights at every size) whose class bias is shifted so that the 640 handle
keeps ~8 candidates per frame at conf 0.25, and a seeded ShuffleNetV2 classifier.  Per handle: the time per call of `rounds`
rounds of `steps` calls after `warmup` calls, the handles alternating inside a round (best and all rounds, frames/s from the
best), once with the classifier (the whole pipeline: its ROI stage follows the boxes a random-weight detector happens to
draw, whose count and size differ between the input shapes) and once on a handle without one (`front_*`: letterbox, detector
and NMS, what the input shape changes); the launch list of one profiled call (count, the fused whole-module launches by name,
and the launches' own event times summed per stage), the modules of the square handle's list that the rectangular handle runs
on the layer plan instead, and the kept boxes per frame.  Nothing is asserted.
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

SIZES = [(640, 640), (384, 640), (320, 640)]
FUSED = ("c2f<", "s2conv", "sppf<", "bottleneck3x3x2<", "head_fused<", "stem_block")   # launches that cover more than one layer


def _time(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def _stages(recs):
    """the launches' event times per stage; a call's launches come in pipeline order: letterbox, detector, nms, roi_resize, classifier"""
    out, after_roi = {}, False
    for r in recs:
        n = r["name"]
        k = "letterbox" if n.startswith("letterbox") else "nms" if n == "nms" else "roi_resize" if n.startswith("roi_resize") else \
            "classifier" if after_roi else "detector"
        after_roi = after_roi or k == "roi_resize"
        out[k] = round(out.get(k, 0.0) + float(r["ms"]), 4)
    return out


def _name(s):
    return f"{s[0]}x{s[1]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from litepi import Engine, ncnn_export, synth
    from litepi.backend import random_shufflenet_state

    B, H, W = a.frames, 1080, 1920
    distinct = min(B, 16)
    base = synth.config4_images(distinct, seed=2, size=1920, grain=8)[:, :H]
    frames = np.ascontiguousarray(np.concatenate([base] * (-(-B // distinct)))[:B])
    d_frames = torch.from_numpy(frames).cuda()
    dd = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    cls_state = random_shufflenet_state(58, seed=3)
    tmp = tempfile.mkdtemp(prefix="rect_bench_")
    res = dict(workload=f"{B} x 1080x1920 device-resident BGR frames per lp_run_batch_device call, fp16, handles of capacity {B}, conf 0.25")
    for preset in ("v1", "v2"):
        files = {}
        for s in SIZES:
            p, b = os.path.join(tmp, f"{preset}_{_name(s)}.param"), os.path.join(tmp, f"{preset}_{_name(s)}.bin")
            ncnn_export.export_detector(p, b, preset, seed=77, cls_bias=0.0, size=s[0] if s[0] == s[1] else s)
            files[s] = (p, b)
        # calibration on the square handle: ~8 candidates per frame at conf 0.25; the same shift for every size
        e = Engine(precision="fp16", max_batch=distinct, max_det=300, num_classes=58)
        e.load_detector(*files[(640, 640)])
        lb = np.stack([e.test_letterbox(f)[0] for f in base])
        sc = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
        e.close()
        k = 8 * distinct
        mid = 0.5 * (np.log(sc[k - 1] / (1 - sc[k - 1])) + np.log(sc[k] / (1 - sc[k])))
        engines, fronts = {}, {}
        for s in SIZES:
            ncnn_export.shift_cls_bias(*files[s], float(np.log(0.25 / 0.75) - mid))
            e = Engine(precision="fp16", max_batch=B, max_det=300, num_classes=58, det_input=s[0] if s[0] == s[1] else s)
            e.load_detector(*files[s])
            e.load_classifier(cls_state)
            engines[s] = e
            e = Engine(precision="fp16", max_batch=B, max_det=300, num_classes=58, det_input=s[0] if s[0] == s[1] else s)
            e.load_detector(*files[s])
            fronts[s] = e

        def call(s):
            engines[s].run_batch_device(d_frames.data_ptr(), B, H, W, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())

        def front(s):
            fronts[s].run_batch_device(d_frames.data_ptr(), B, H, W, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())

        out, lists, stage_ms = {}, {}, {}
        for s in SIZES:   # eager call, captured call, then one profiled call for the launch list
            call(s); call(s); front(s); front(s)
            engines[s].synchronize()
            fronts[s].synchronize()
            engines[s].profile_next(True)
            call(s)
            engines[s].synchronize()
            recs = engines[s].profile_read()
            lists[s] = [r["name"] for r in recs]
            stage_ms[s] = _stages(recs)
        times, ftimes = {s: [] for s in SIZES}, {s: [] for s in SIZES}
        for _ in range(a.rounds):
            for s in SIZES:
                times[s].append(_time(lambda: call(s), a.steps, a.warmup))
            for s in SIZES:
                ftimes[s].append(_time(lambda: front(s), a.steps, a.warmup))
        for s in SIZES:
            call(s)
            engines[s].synchronize()
            kept = dc.cpu().numpy()[:B]
            t = min(times[s])
            fused = sorted(n for n in lists[s] if n.startswith(FUSED))
            out[_name(s)] = dict(ms_per_call=round(t * 1e3, 3), ms_rounds=[round(x * 1e3, 3) for x in times[s]], frames_per_s=round(B / t, 1),
                                 front_ms_per_call=round(min(ftimes[s]) * 1e3, 3), front_ms_rounds=[round(x * 1e3, 3) for x in ftimes[s]],
                                 front_frames_per_s=round(B / min(ftimes[s]), 1),
                                 launches=len(lists[s]), anchors=engines[s].num_anchors, fused_launches=fused,
                                 profiled_ms_by_stage=stage_ms[s], kept_per_frame_mean=round(float(kept.mean()), 2))
        sq = set(out["640x640"]["fused_launches"])
        for s in SIZES[1:]:
            o = out[_name(s)]
            o["fused_on_640_only"] = sorted(sq - set(o["fused_launches"]))
            o["speedup_vs_640"] = round(out["640x640"]["ms_per_call"] / o["ms_per_call"], 3)
            o["front_speedup_vs_640"] = round(out["640x640"]["front_ms_per_call"] / o["front_ms_per_call"], 3)
        for e in list(engines.values()) + list(fronts.values()):
            e.close()
        res[preset] = out
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
