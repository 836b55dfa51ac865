#!/usr/bin/env python3
"""Tiled inference throughput (DESIGN.md "Tiled inference").

    python tools/tile_bench.py [--frames 3] [--steps 50] [--warmup 10] [--out profiles/tile_bench.json]
                               [--view_match iou|ios] [--view_merge nms|union] [--conf 0.25] [--skip_profile]

Times lp_run_tiled_device on TT100K-shape 2048x2048 frames (synth.config4_images, grain 8) in fp16 with overlap 128 and
full_frame 1 -- 17 views per frame -- on a 64-view handle, and in the same process, as the baseline, lp_run_batch_device on
the same 640x640 views (each frame's letterbox and 16 crops, cut on the host).  Both sides are timed alike: two alternating
rounds each, the better round reported, and the kept counts of both are printed.  Seeded synthetic v1 detector whose class bias puts ~8 candidates per view over conf 0.25
(bench.py's calibration); random ShuffleNetV2 classifier.  One profiled call per conf (0.25, 0.001) gives the new launches'
times (lp_profile_read).  Prints one JSON line.

--view_match / --view_merge set the frame NMS's merge of the views (Engine.set_view_merge; absent: the handle is not touched).
For a kernel trace of frame_nms at ONE confidence, --conf sets the confidence of the timed tiled calls and
--skip_profile leaves out the two profiled calls at 0.25 and 0.001:
    rocprofv3 --kernel-trace --stats -d out -- python tools/tile_bench.py --conf 0.001 --skip_profile --steps 20 --warmup 5
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

HBM_TBPS = 8.0   # MI355X HBM3E peak


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--view_match", choices=["iou", "ios"], default=None)
    ap.add_argument("--view_merge", choices=["nms", "union"], default=None)
    ap.add_argument("--conf", type=float, default=0.25, help="confidence of the timed tiled calls")
    ap.add_argument("--skip_profile", action="store_true", help="no profiled calls at 0.25 / 0.001 (for a kernel trace at --conf alone)")
    a = ap.parse_args()
    import torch
    from litepi import Engine, ncnn_export, synth
    from litepi.backend import random_shufflenet_state

    tmp = tempfile.mkdtemp(prefix="tile_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    frames = synth.config4_images(a.frames, seed=2, size=2048, grain=8)
    n_views = 17 * a.frames
    e = Engine(precision="fp16", max_batch=64, max_det=300, num_classes=58)
    e.load_detector(p, b)
    views = np.stack([frames[0][y:y + 640, x:x + 640] for y in (0, 512, 1024, 1408) for x in (0, 512, 1024, 1408)])
    s = np.sort(e.detect_raw(views)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    k = 8 * len(views)
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
    e.load_detector(p, b)
    e.load_classifier(random_shufflenet_state(58, seed=3))
    if a.view_match is not None or a.view_merge is not None:
        e.set_view_merge(a.view_match or "iou", a.view_merge or "nms")
    B = a.frames
    d_frames = torch.from_numpy(frames).cuda()
    # baseline input: the very views the tiled path makes of these frames (the letterboxed frame + its 16 crops each), so both
    # sides see the same pixels and about the same candidates
    base = []
    for f in frames:
        base.append(e.test_letterbox(f)[0])
        base += [f[y:y + 640, x:x + 640] for y in (0, 512, 1024, 1408) for x in (0, 512, 1024, 1408)]
    d_views = torch.from_numpy(np.ascontiguousarray(np.stack(base))).cuda()
    dd = torch.zeros(64 * 300 * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * 64, dtype=torch.int32, device="cuda")

    def tiled(conf=a.conf):
        e.run_tiled_device(d_frames.data_ptr(), B, 2048, 2048, conf, 0.45, 50, dd.data_ptr(), dc.data_ptr(), 128, True)

    def plain():
        e.run_batch_device(d_views.data_ptr(), n_views, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())

    # both sides timed alike: two alternating rounds each, the better round of each side
    t_tiled, t_plain = [], []
    for _ in range(2):
        t_tiled.append(_time(tiled, a.steps, a.warmup))
        t_plain.append(_time(plain, a.steps, a.warmup))
    plain()
    e.synchronize()
    base_kept = dc.cpu().numpy()[n_views:2 * n_views]
    prof = {}
    for conf in () if a.skip_profile else (0.25, 0.001):
        tiled(conf)
        e.synchronize()
        e.profile_next(True)
        tiled(conf)
        e.synchronize()
        kept = dc.cpu().numpy()[B:2 * B].tolist()
        recs = {r["name"]: r for r in e.profile_read() if r["name"] in ("tile_crop_u8", "letterbox_u8", "view_sort", "frame_nms")}
        prof[str(conf)] = {n: dict(ms=round(r["ms"], 4), gbs=round(r["bytes"] / (r["ms"] * 1e6), 1) if r["bytes"] else None)
                           for n, r in recs.items()}
        prof[str(conf)]["kept_per_frame"] = kept
    tiled()
    e.synchronize()
    kept_timed = dc.cpu().numpy()[B:2 * B].tolist()
    e.close()
    crop = prof.get("0.25", {}).get("tile_crop_u8", {})
    t_plain_rounds = t_plain
    t_best, t_plain = min(t_tiled), min(t_plain)
    res = dict(workload=f"{B} x 2048x2048 frames, fp16, overlap 128, full_frame 1 ({n_views} views), 64-view handle",
               view_merge=[a.view_match or "iou", a.view_merge or "nms"], conf=a.conf, kept_per_frame=kept_timed,
               tiled_ms_per_call=round(t_best * 1e3, 3), tiled_ms_rounds=[round(t * 1e3, 3) for t in t_tiled],
               tiled_frames_per_s=round(B / t_best, 1),
               baseline_ms_per_call=round(t_plain * 1e3, 3), baseline_ms_rounds=[round(t * 1e3, 3) for t in t_plain_rounds],
               baseline_views_per_s=round(n_views / t_plain, 1),
               baseline_kept_per_view_mean=round(float(base_kept.mean()), 2), baseline_kept_total=int(base_kept.sum()),
               target_frames_per_s=round(0.85 * n_views / t_plain / 17, 1),
               ratio_vs_target=round((B / t_best) / (n_views / t_plain / 17), 3),
               crop_hbm_fraction=round(crop["gbs"] / (HBM_TBPS * 1e3), 3) if crop.get("gbs") else None,
               profile=prof)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
