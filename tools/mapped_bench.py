#!/usr/bin/env python3
"""What a table-driven view gather costs against the window gather.

    python tools/mapped_bench.py [--steps 30] [--warmup 5] [--out profiles/mapped_bench.json]

16 views of det_input 640 out of two device-resident 1080p BGR frames (8 views per frame) through lp_run_mapped_device /
lp_run_views_device, fp16, conf 0.25.  Four view lists of the same source footprint (640 x 640 frame pixels per view, at the
same eight places of the frame):

windows    8 windows {x, y, 640, 640} per frame: window_views_u8, the letterbox core's copy branch
crop       8 integer crop maps (litepi.lens.crop_map) at the same origins: the same bytes through the table
rotation   the same places turned by 7 degrees
fisheye    8 rectified pinhole views (hfov 60) out of the frame read as a 150 degree equidistant fisheye (lens.pinhole_from_fisheye)

Per list: the eager time of the gather launch and of map_candidates from the handle's profiler (lp_profile_next: events around
each launch of an eager step), median and p10 / p90 over `steps` profiled steps after `warmup` unprofiled ones, and the
algorithmic bytes: table (8 B per view pixel) + source footprint (the bounding rectangle of each view's positions inside the
frame, 3 B per pixel) + view (3 B per view pixel); the profiler's own booking (whole frames) is recorded beside it.  No
threshold: nobody had measured a table-driven gather on this chip.  Seeded synthetic v1 detector calibrated to ~8 candidates per
640 x 640 noise view (bench.py's calibration), no classifier.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "yolo-litepi_amd"))

S, H, W, B, PER = 640, 1080, 1920, 2, 8
ORIGINS = [(40, 20), (660, 30), (1270, 10), (120, 430), (640, 220), (1200, 436), (333, 111), (901, 401)]   # x, y of the 640 x 640 places


def _q(v):
    v = np.asarray(v, dtype=np.float64) * 1e3
    return dict(median_us=round(float(np.median(v)), 2), p10_us=round(float(np.percentile(v, 10)), 2), p90_us=round(float(np.percentile(v, 90)), 2), n=len(v))


def _model():
    from litepi import Engine, ncnn_export
    tmp = tempfile.mkdtemp(prefix="mapped_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    imgs = np.random.default_rng(7).integers(0, 256, (16, S, S, 3), dtype=np.uint8)
    e = Engine(precision="fp16", max_batch=16, max_det=300, num_classes=58)
    e.load_detector(p, b)
    s = np.sort(e.detect_raw(imgs)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    e.close()
    k = 8 * 16
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
    return p, b


def _rotated(x0, y0, degrees):
    """the 640 x 640 place at (x0, y0) turned about its centre"""
    c = (S - 1) / 2.0
    j, i = np.meshgrid(np.arange(S) - c, np.arange(S) - c, indexing="ij")
    a = np.radians(degrees)
    xy = np.empty((S, S, 2))
    xy[..., 0] = x0 + c + np.cos(a) * i - np.sin(a) * j
    xy[..., 1] = y0 + c + np.sin(a) * i + np.cos(a) * j
    return xy.astype(np.float32)


def _footprint_bytes(xy):
    x = np.clip(xy[..., 0], 0, W - 1)
    y = np.clip(xy[..., 1], 0, H - 1)
    return float((np.floor(x.max()) + 2 - np.floor(x.min())) * (np.floor(y.max()) + 2 - np.floor(y.min())) * 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from litepi import Engine, lens
    p, b = _model()
    frames = np.random.default_rng(11).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    d_img = torch.from_numpy(frames).cuda()
    dd = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e = Engine(precision="fp16", max_batch=B * PER, max_det=300, num_classes=58)
    e.load_detector(p, b)
    f_fish = (W / 2.0) / np.radians(75.0)   # 150 degrees across the frame's width
    K = np.array([[f_fish, 0, (W - 1) / 2.0], [0, f_fish, (H - 1) / 2.0], [0, 0, 1.0]])
    tables = {"crop": [lens.crop_map(S, x, y) for x, y in ORIGINS],
              "rotation": [_rotated(x, y, 7.0) for x, y in ORIGINS],
              "fisheye": [lens.pinhole_from_fisheye(S, K, (), yaw=yaw, pitch=pitch, hfov=60.0)
                          for yaw, pitch in ((-45, 0), (-15, 0), (15, 0), (45, 0), (-30, 12), (0, 12), (30, 12), (0, -12))]}
    res = {"workload": f"{B} x {H}x{W} BGR frames on the device, {PER} views of {S}x{S} each = {B * PER} views per launch, fp16 v1 detector, conf 0.25",
           "lists": {}}
    view_bytes, table_bytes = B * PER * S * S * 3.0, B * PER * S * S * 8.0
    for name in ("windows", "crop", "rotation", "fisheye"):
        e.map_clear()
        if name == "windows":
            views = [(x, y, S, S) for x, y in ORIGINS]
            step = lambda: e.run_views_device(d_img.data_ptr(), B, H, W, views, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())   # noqa: E731
            algo = view_bytes + B * PER * S * S * 3.0
        else:
            ids = [e.map_add(t, H, W) for t in tables[name]]
            step = lambda: e.run_mapped_device(d_img.data_ptr(), B, H, W, [], ids, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())   # noqa: E731
            algo = table_bytes + view_bytes + B * sum(_footprint_bytes(t) for t in tables[name])
        for _ in range(a.warmup):
            step()
        e.synchronize()
        per, booked = {}, {}
        for _ in range(a.steps):
            e.profile_next(True)
            step()
            e.synchronize()
            for r in e.profile_read():
                if r["name"] in ("map_views_u8", "window_views_u8", "map_candidates"):
                    per.setdefault(r["name"], []).append(r["ms"])
                    booked[r["name"]] = r["bytes"]
        gather = "window_views_u8" if name == "windows" else "map_views_u8"
        entry = {"gather": gather, "gather_time": _q(per[gather]), "algorithmic_bytes": algo, "profiler_bytes": booked[gather],
                 "gather_gb_per_s": round(algo / (float(np.median(per[gather])) * 1e-3) / 1e9, 1),
                 "kept_after_nms": int(dc.cpu().numpy()[B:2 * B].sum())}
        if "map_candidates" in per:
            entry["map_candidates_time"] = _q(per["map_candidates"])
        res["lists"][name] = entry
    e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
