#!/usr/bin/env python3
"""What the device-side sign inventory costs behind the pipeline and the tracker.

    python tools/inventory_bench.py [--steps 200] [--warmup 20] [--out profiles/inventory_bench.json]

One process, the bench's batch (64 x 640^2, fp16, conf 0.25).  For each of three shapes of the same 64 frames -- 64 streams
x 1 frame, 8 streams x 8 frames, 1 stream x 64 frames -- "pipeline + tracker" and "pipeline + tracker + inventory (crops)"
alternate step by step, every step synchronised; medians with p10 / p90.  The inventory launches' own time comes from events
around lp_inventory_device on the handle's stream.  The yardstick is what it replaces: downloading both record buffers and
the crop buffer of the call and running the NumPy loop of tests/inventory_ref.py on the host.

"approaching": the case LP_BEST_AREA is worst at, model-free.  Eight signs per frame grow from frame to frame, so every
sighting is a new best and copies its crop into the gallery; consecutive calls carry other track ids, so every call also
closes and logs the eight signs of the call before.  Events around lp_inventory_device alone, the three shapes.

Seeded synthetic v1 detector whose class bias puts ~8 candidates per frame over conf 0.25 (bench.py's calibration), random
ShuffleNetV2 classifier, noise frames, as tools/track_bench.py.  Prints one JSON line.

The kernels' own time as the profiler sees it (a run of its own, 20 steps):

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/inventory_bench.py --steps 20 --warmup 5 --host-reps 1
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


def approaching(e, st, torch, shapes, reps):
    """model-free: 8 growing signs per frame, 64 frames per call, every record has a crop; two sets of ids alternate"""
    from litepi._ffi import DET_DTYPE, TRACK_DTYPE
    B, MD, K = 64, e.cfg.max_det, 8
    S = e.cfg.cls_input
    rng = np.random.default_rng(5)
    e.test_set_rois(rng.integers(0, 256, (B * K, S, S, 3), dtype=np.uint8), np.repeat(np.arange(B), K), np.tile(np.arange(K), B))
    out = {}
    for name, sid in shapes.items():
        nth = np.zeros(B, np.int64)   # the frame's position within its stream
        seen = {}
        for b, s in enumerate(sid.tolist()):
            nth[b] = seen.get(s, 0)
            seen[s] = nth[b] + 1
        dets = np.zeros((B, MD), dtype=DET_DTYPE)
        for i in range(K):
            size = (20.0 + 2.0 * nth + i).astype(np.float32)
            dets["x1"][:, i], dets["y1"][:, i] = 60.0 * i, 40.0
            dets["x2"][:, i], dets["y2"][:, i] = 60.0 * i + size, 40.0 + size
            dets["det_conf"][:, i], dets["cls_class"][:, i], dets["cls_conf"][:, i] = 0.9, i, 0.8
        bufs = []
        for gen in (0, 1):
            tr = np.zeros((B, MD), dtype=TRACK_DTYPE)
            for i in range(K):
                tr["track_id"][:, i], tr["slot"][:, i], tr["hits"][:, i] = 1 + gen * K + i, i, 3 + nth
                tr["voted_class"][:, i], tr["voted_conf"][:, i], tr["vote_weight"][:, i] = i, 0.8, 1.0
            bufs.append(torch.from_numpy(tr.view(np.uint8).reshape(-1).copy()).cuda())
        dd = torch.from_numpy(dets.view(np.uint8).reshape(-1).copy()).cuda()
        dc = torch.full((B,), K, dtype=torch.int32, device="cuda")
        e.tracker_create(n_streams=B, max_tracks=64)
        e.inventory_create(max_signs=1 << 16, best="area")
        ev = []
        for r in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            e.inventory_device(dd.data_ptr(), dc.data_ptr(), bufs[r % 2].data_ptr(), B, sid, crops=True)
            e1.record(st)
            e.synchronize()
            if r >= 5:
                ev.append(e0.elapsed_time(e1))
        signs, _, dropped = e.inventory_drain(crops=False)
        out[name] = dict(inventory_events=_q(ev), crops_copied_per_call=B * K, signs_logged=int(len(signs)), dropped=int(dropped))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    import inventory_ref as V
    from litepi import Engine, ncnn_export
    from litepi._ffi import DET_DTYPE, TRACK_DTYPE
    from litepi.backend import random_shufflenet_state

    tmp = tempfile.mkdtemp(prefix="inventory_bench_")
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
    tcfg = dict(n_streams=B, max_tracks=64)
    icfg = dict(max_signs=1 << 16, best=V.BEST_AREA)
    shapes = {"64x1": np.arange(B, dtype=np.int32), "8x8": np.repeat(np.arange(8, dtype=np.int32), 8), "1x64": np.zeros(B, np.int32)}
    res = dict(workload="64 x 640x640 frames, fp16, synthetic v1 detector + ShuffleNetV2, conf 0.25, max_det 300, max_tracks 64, "
                        "LP_BEST_AREA, keep_crops 1")

    def tracked():
        e.run_batch_device(d_img.data_ptr(), B, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
        e.track_device(dd.data_ptr(), dc.data_ptr(), B, dt.data_ptr(), sid)

    for name, sid in shapes.items():
        e.tracker_create(**tcfg)
        e.inventory_create(**icfg)

        def inventoried():
            tracked()
            e.inventory_device(dd.data_ptr(), dc.data_ptr(), dt.data_ptr(), B, sid, crops=True)

        t_trk, t_inv = _alternate(tracked, inventoried, e.synchronize, a.steps, a.warmup)
        signs, _, dropped = e.inventory_drain(crops=False)
        ev = []
        for _ in range(50):
            tracked()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            e.inventory_device(dd.data_ptr(), dc.data_ptr(), dt.data_ptr(), B, sid, crops=True)
            e1.record(st)
            e.synchronize()
            ev.append(e0.elapsed_time(e1))
        kept = dc.cpu().numpy()[:B]
        # the yardstick: both record buffers and the crop buffer to the host + the NumPy loop, same call
        ref = V.InventoryRef(MD, tcfg, icfg)
        th = []
        for _ in range(a.host_reps):
            tracked()
            e.synchronize()
            t0 = time.perf_counter()
            dets = dd.cpu().numpy().view(DET_DTYPE).reshape(B, MD)
            tracks = dt.cpu().numpy().view(TRACK_DTYPE).reshape(B, MD)
            counts = dc.cpu().numpy()[:B]
            crops, img, slot = e.debug_rois()
            ref.feed(dets, tracks, counts, sid, crops=V.rois_to_crops(crops, img, slot))
            ref.drain()
            th.append((time.perf_counter() - t0) * 1e3)
        res[name] = dict(pipeline_plus_tracker=t_trk, pipeline_plus_tracker_plus_inventory=t_inv,
                         added_ms=round(t_inv["median_ms"] - t_trk["median_ms"], 4), inventory_events=_q(ev), host_download_plus_numpy=_q(th),
                         kept_total=int(kept.sum()), signs_logged=int(len(signs)), dropped=int(dropped))
    res["approaching"] = approaching(e, st, torch, shapes, 50)
    e.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
