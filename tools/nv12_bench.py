#!/usr/bin/env python3
"""What NV12 input costs and buys.

    python tools/nv12_bench.py [--steps 200] [--warmup 20] [--large-steps 200] [--out profiles/nv12_bench.json]

Both sides of every comparison run in this one process on the same frames, alternating step by step, warmed up; every step
is synchronised and the medians are reported:

  converter       nv12_to_bgr alone at 64 x 640^2 and 32 x 2048^2, from lp_profile_read (the launch's own events): time, achieved
                  bytes/s over its algorithmic 4.5 B per pixel and the share of the 8 TB/s HBM peak; next to it, measured the
                  same way in the same session, the project's other byte movers (tile_crop_u8, letterbox_u8)
  device          lp_run_batch_device, 64 x 640^2, fp16, one handle: NV12 step against BGR step
  host            lp_run_batch from host frames, 64 x 640^2 (the upload-inclusive situation): NV12 against BGR
  large           32 x 2048^2 through lp_run_batch_device: the staging pass next to the letterbox

Seeded synthetic v1 detector whose class bias puts ~8 candidates per frame over conf 0.25 (bench.py's calibration), random
ShuffleNetV2 classifier.  The NV12 frames are made from BGR noise with a plain BT.601 forward transform; the BGR side gets
the library's own conversion of them (lp_test_convert_frames), so both sides see the same pixels.  Prints one JSON line.
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


def bgr_to_nv12(img):
    H, W = img.shape[:2]
    b, g, r = (img[..., k].astype(np.float32) for k in range(3))
    y = 16.0 + 0.256788 * r + 0.504129 * g + 0.097906 * b
    u = 128.0 - 0.148223 * r - 0.290993 * g + 0.439216 * b
    v = 128.0 + 0.439216 * r - 0.367788 * g - 0.071427 * b
    sub = lambda p: p.reshape(H // 2, 2, W // 2, 2).mean(axis=(1, 3))   # noqa: E731
    out = np.empty((H * 3 // 2, W), np.uint8)
    out[:H] = np.clip(np.rint(y), 0, 255)
    out[H:] = np.clip(np.rint(np.stack([sub(u), sub(v)], -1)), 0, 255).reshape(H // 2, W)
    return out


def _alternate(fn_a, fn_b, sync, steps, warmup):
    """a, b, a, b ... every step synchronised; medians and the 10th / 90th percentiles in ms"""
    ta, tb = [], []
    for i in range(warmup + steps):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= warmup:
                acc.append((time.perf_counter() - t0) * 1e3)
    q = lambda t: dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(np.percentile(t, 10)), 4),   # noqa: E731
                       p90_ms=round(float(np.percentile(t, 90)), 4), steps=len(t))
    return q(ta), q(tb)


def _profiled(e, fn, names, reps):
    """median per-launch time of the named kernel families over `reps` profiled (eager) calls"""
    acc = {}
    for _ in range(reps):
        e.profile_next(True)
        fn()
        e.synchronize()
        for r in e.profile_read():
            if r["name"] in names:
                acc.setdefault(r["name"], []).append((r["ms"], r["bytes"]))
    out = {}
    for n, v in acc.items():
        ms = float(np.median([x[0] for x in v]))
        by = v[0][1]
        out[n] = dict(median_ms=round(ms, 5), bytes=by, tb_per_s=round(by / (ms * 1e9), 3) if ms > 0 else None,
                      hbm_fraction=round(by / (ms * 1e9) / HBM_TBPS, 3) if ms > 0 else None, launches=len(v))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--large-steps", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state

    tmp = tempfile.mkdtemp(prefix="nv12_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    rng = np.random.default_rng(7)
    B = 64
    nv = np.stack([bgr_to_nv12(rng.integers(0, 256, (640, 640, 3), dtype=np.uint8)) for _ in range(B)])
    e = Engine(precision="fp16", max_batch=B, max_det=300, num_classes=58)
    e.load_detector(p, b)
    bgr = e.test_convert_frames(nv, B, 640, 640)
    s = np.sort(e.detect_raw(bgr[:16])[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    k = 8 * 16
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
    e.load_detector(p, b)
    e.load_classifier(random_shufflenet_state(58, seed=3))
    dd = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    d_nv, d_bgr = torch.from_numpy(nv).cuda(), torch.from_numpy(bgr).cuda()
    nv_list, bgr_list = list(nv), list(bgr)
    res = dict(workload="64 x 640x640 and 32 x 2048x2048 frames, fp16, synthetic v1 detector + ShuffleNetV2, conf 0.25")

    def dev(fmt, buf, n=B, H=640, W=640):
        def step():
            e.set_input_format(fmt)
            e.run_batch_device(buf.data_ptr(), n, H, W, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
        return step

    def host(fmt, frames):
        def step():
            e.set_input_format(fmt)
            e.run_batch(frames, 0.25, 0.45, 50)
        return step

    # ---- device-resident frames, 64 x 640^2
    t_nv, t_bgr = _alternate(dev("nv12", d_nv), dev("bgr", d_bgr), e.synchronize, a.steps, a.warmup)
    kept_nv = dc.cpu().numpy()[:B].copy()
    dev("bgr", d_bgr)(); e.synchronize()
    kept_bgr = dc.cpu().numpy()[:B].copy()
    res["device_64x640"] = dict(nv12=t_nv, bgr=t_bgr, nv12_minus_bgr_ms=round(t_nv["median_ms"] - t_bgr["median_ms"], 4),
                                kept_total=int(kept_bgr.sum()), same_counts=bool(np.array_equal(kept_nv, kept_bgr)))
    res["converter_64x640"] = _profiled(e, dev("nv12", d_nv), ("nv12_to_bgr",), 50)
    # ---- host frames, 64 x 640^2 (the upload is part of the step)
    t_nv, t_bgr = _alternate(host("nv12", nv_list), host("bgr", bgr_list), lambda: None, a.steps, a.warmup)
    res["host_64x640"] = dict(nv12=t_nv, bgr=t_bgr, bgr_over_nv12=round(t_bgr["median_ms"] / t_nv["median_ms"], 3),
                              nv12_images_per_s=round(B / t_nv["median_ms"] * 1e3, 1), bgr_images_per_s=round(B / t_bgr["median_ms"] * 1e3, 1))
    e.close()
    del d_nv, d_bgr

    # ---- 32 x 2048^2: the staging pass next to the letterbox, and the crop gather as this session's byte-mover yardstick
    from litepi import synth
    BL = 32
    big = synth.config4_images(4, seed=2, size=2048, grain=8)
    nv_big = np.stack([bgr_to_nv12(big[i % 4]) for i in range(BL)])
    e = Engine(precision="fp16", max_batch=max(BL, 34), max_det=300, num_classes=58)
    e.load_detector(p, b)
    e.load_classifier(random_shufflenet_state(58, seed=3))
    d_nv = torch.from_numpy(nv_big).cuda()
    bgr_big = np.concatenate([e.test_convert_frames(nv_big[i:i + 8], 8, 2048, 2048) for i in range(0, BL, 8)])
    d_bgr = torch.from_numpy(bgr_big).cuda()
    t_nv, t_bgr = _alternate(dev("nv12", d_nv, BL, 2048, 2048), dev("bgr", d_bgr, BL, 2048, 2048), e.synchronize, a.large_steps, a.warmup)
    res["device_32x2048"] = dict(nv12=t_nv, bgr=t_bgr, nv12_minus_bgr_ms=round(t_nv["median_ms"] - t_bgr["median_ms"], 4))
    res["converter_32x2048"] = _profiled(e, dev("nv12", d_nv, BL, 2048, 2048), ("nv12_to_bgr", "letterbox_u8"), 50)

    def tiled():   # two frames, 34 views: the crop gather measured in this session
        e.set_input_format("bgr")
        e.run_tiled_device(d_bgr.data_ptr(), 2, 2048, 2048, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr(), 128, True)
    tiled(); e.synchronize()
    res["yardstick_crop_gather"] = _profiled(e, tiled, ("tile_crop_u8",), 50)
    e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
