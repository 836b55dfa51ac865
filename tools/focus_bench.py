#!/usr/bin/env python3
"""Focus views: what the device-side plan costs, and what it finds.

    python tools/focus_bench.py [--frames 3] [--steps 50] [--warmup 10] [--rounds 3] [--out profiles/focus_bench.json]

1. Frames/s on `frames` 2048x2048 frames resident in HBM, one process, fp16, det_input 640, a seeded v1 detector with
   tile_bench.py's calibration, one tracker stream per frame fed by the pipeline's own records before the timed rounds.
   The rounds alternate: lp_run_batch_device (1 view), lp_run_focus_device with slots = 3 (4 views), lp_run_views_device with a
   fixed list of the whole frame + 3 native windows (the yardstick: the same view count without a plan) and
   lp_run_tiled_device (17 views).  Reported: the per-call time of every round, the focus call minus the yardstick, the
   event time of the focus_plan launch (lp_profile_next) and, beside it, the time of an lp_track_device call (its launch
   carries no events: 100 calls back to back behind one synchronise).
2. With the reference's real v1 weights staged under oracle/_ref: views_bench.py's sign scene with the pasted signs moving a
   few pixels per frame over 20 frames; signs found per frame (IoU >= 0.5) by letterbox, focus (3 slots) and tiled inference.
   Printed, nothing is asserted.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "yolo-litepi_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import views_bench as VB  # noqa: E402


def moving_scene(n_frames):
    """the sign scene's crops on its background, every sign moving (2, 1) pixels a frame"""
    img, rects = VB._sign_scene()
    crops = [img[y1:y2, x1:x2].copy() for x1, y1, x2, y2 in rects]
    bg, _ = VB._sign_scene()
    for x1, y1, x2, y2 in rects:   # the background under a sign: its surroundings' mean
        bg[y1:y2, x1:x2] = bg[max(y1 - 4, 0):y1, x1:x2].mean(axis=(0, 1)).astype(np.uint8)
    frames, truth = [], []
    for k in range(n_frames):
        f = bg.copy()
        moved = []
        for c, (x1, y1, x2, y2) in zip(crops, rects):
            f[y1 + k:y2 + k, x1 + 2 * k:x2 + 2 * k] = c
            moved.append((x1 + 2 * k, y1 + k, x2 + 2 * k, y2 + k))
        frames.append(f)
        truth.append(moved)
    return frames, truth


def real_weights_recall(n_frames=20):
    if not all(os.path.exists(p) for p in VB._REAL):
        return None
    import torch
    from litepi import HybridPipeline
    from litepi.backend import random_shufflenet_state
    frames, truth = moving_scene(n_frames)
    cls_path = os.path.join(tempfile.mkdtemp(prefix="focus_bench_"), "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in random_shufflenet_state(58, seed=3).items()}, cls_path)
    out = {}
    modes = (("letterbox", dict(max_batch=1)), ("focus_3_slots", dict(max_batch=4, track=True, focus=3)),
             ("tiled_overlap_128", dict(max_batch=17, tile_overlap=128)))
    for mode, kw in modes:
        pipe = HybridPipeline(*VB._REAL, cls_path, "shufflenetv2", num_classes=58, precision="fp16", max_det=300, **kw)
        found, placed = [], []
        try:
            for f, rects in zip(frames, truth):
                res, _ = pipe.run_batch([f], 0.25, 0.45, 50)[0]
                found.append(sum(any(VB._iou(rc, r["bbox"]) >= 0.5 for r in res) for rc in rects))
                if "focus" in kw:
                    placed.append(pipe.last_focus_views[0])
        finally:
            pipe.close()
        out[mode] = dict(signs_found_per_frame=found, mean=round(float(np.mean(found)), 2), last_frame=found[-1])
        if placed:
            out[mode]["windows_last_frame"] = placed[-1]
    out["signs_pasted"] = len(truth[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--recall-only", action="store_true", help="only part 2 (the real v1 weights on the moving sign scene)")
    a = ap.parse_args()
    if a.recall_only:
        print(json.dumps(dict(real_v1_moving_signs=real_weights_recall())))
        return
    import torch
    from litepi import Engine, ncnn_export, synth
    from litepi.backend import random_shufflenet_state

    tmp = tempfile.mkdtemp(prefix="focus_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    frames = synth.config4_images(a.frames, seed=2, size=2048, grain=8)
    B, H, W = a.frames, 2048, 2048
    e = Engine(precision="fp16", max_batch=64, max_det=300, num_classes=58)
    e.load_detector(p, b)
    views = np.stack([frames[0][y:y + 640, x:x + 640] for y in (0, 512, 1024, 1408) for x in (0, 512, 1024, 1408)])
    s = np.sort(e.detect_raw(views)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    k = 8 * len(views)
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
    e.load_detector(p, b)
    e.load_classifier(random_shufflenet_state(58, seed=3))
    e.tracker_create(n_streams=B, max_tracks=64)
    e.focus_create(slots=3)
    d_frames = torch.from_numpy(frames).cuda()
    dd = torch.zeros(64 * 300 * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * 64, dtype=torch.int32, device="cuda")
    dt = torch.zeros(64 * 300 * 32, dtype=torch.uint8, device="cuda")
    dv = torch.zeros(B * 3 * 4, dtype=torch.int32, device="cuda")
    ids = list(range(B))
    fixed = ["full", (0, 0, 640, 640), (700, 700, 640, 640), (1408, 1408, 640, 640)]
    args = (0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())

    def run_focus():
        e.run_focus_device(d_frames.data_ptr(), B, H, W, *args, stream_ids=ids, dev_views=dv.data_ptr())

    def run_track():
        e.track_device(dd.data_ptr(), dc.data_ptr(), B, dt.data_ptr(), ids)

    modes = {"letterbox_1_view": lambda: e.run_batch_device(d_frames.data_ptr(), B, H, W, *args),
             "focus_3_slots_4_views": run_focus,
             "views_fixed_4_views": lambda: e.run_views_device(d_frames.data_ptr(), B, H, W, fixed, *args),
             "tiled_overlap_128_17_views": lambda: e.run_tiled_device(d_frames.data_ptr(), B, H, W, *args, 128, True)}
    for _ in range(4):   # the tracker's state: the pipeline's own records, a few frames of it
        run_focus()
        run_track()
    e.synchronize()
    live = [len(e.tracker_snapshot(s)["tracks"]) for s in ids]
    times = {n: [] for n in modes}
    kept = {}
    for _ in range(a.rounds):
        for n, fn in modes.items():
            times[n].append(VB._time(fn, a.steps, a.warmup))
            e.synchronize()
            kept[n] = dc.cpu().numpy()[B:2 * B].tolist()
    through = {n: dict(ms_rounds=[round(x * 1e3, 3) for x in t], ms_per_call=round(min(t) * 1e3, 3), frames_per_s=round(B / min(t), 1),
                       kept_per_frame=kept[n]) for n, t in times.items()}
    yard = times["views_fixed_4_views"]
    plan_us, track_us = [], []
    launches = {"focus_3_slots_4_views": {}, "views_fixed_4_views": {}}   # name -> per profiled call, the summed event time in us
    for _ in range(9):
        for n in launches:
            e.profile_next(True)
            modes[n]()
            e.synchronize()
            recs = e.profile_read()
            per = {}
            for r in recs:
                per[r["name"]] = per.get(r["name"], 0.0) + r["ms"] * 1e3
            per["all_launches"] = sum(r["ms"] for r in recs) * 1e3
            for name, us in per.items():
                launches[n].setdefault(name, []).append(us)
            if n == "focus_3_slots_4_views":
                plan_us += [r["ms"] * 1e3 for r in recs if r["name"] == "focus_plan"]
        track_us.append(VB._time(run_track, 100, 5) * 1e6)   # (its launch carries no events: 100 calls back to back, one synchronise)
    cost = dict(focus_minus_yardstick_us=round((min(times["focus_3_slots_4_views"]) - min(yard)) * 1e6, 1),
                focus_minus_yardstick_us_rounds=[round((f - y) * 1e6, 1) for f, y in zip(times["focus_3_slots_4_views"], yard)],
                yardstick_spread_us=round((max(yard) - min(yard)) * 1e6, 1),
                focus_plan_event_us_median=round(float(np.median(plan_us)), 2), focus_plan_event_us=[round(x, 2) for x in plan_us],
                track_device_us_per_call_back_to_back=round(float(np.median(track_us)), 2))
    # where the difference goes: the launches of one eager, profiled call of either kind, median event time per kernel family
    # (the families of the detector and the classifier summed under "all_launches" only)
    front = ("focus_plan", "letterbox_u8", "window_views_u8", "focus_mask", "view_sort", "frame_nms", "roi_resize_pil", "all_launches")
    cost["launch_event_us_median"] = {n: {k: round(float(np.median(v)), 2) for k, v in per.items() if k in front} for n, per in launches.items()}
    e.synchronize()
    windows = dv.cpu().numpy().reshape(B, 3, 4).tolist()
    e.close()
    res = dict(workload=f"{B} x 2048x2048 frames per call, fp16, det_input 640, 64-view handle, conf 0.25, one tracker stream per frame",
               live_tracks_per_stream=live, windows_last_call=windows, throughput=through, plan_cost=cost,
               real_v1_moving_signs=real_weights_recall())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
