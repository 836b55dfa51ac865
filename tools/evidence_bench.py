#!/usr/bin/env python3
"""What the evidence store costs behind the pipeline, the tracker and the inventory.

    python tools/evidence_bench.py [--steps 100] [--warmup 10] [--out profiles/evidence_bench.json]

One process, the bench's batch (64 x 640^2, fp16, conf 0.25), two handles with the same models: one whose inventory has an
evidence store and one without.  For each picture side E in (64, 128) and each of three shapes of the same 64 frames -- 64
streams x 1 frame, 8 streams x 8 frames, 1 stream x 64 frames -- "pipeline + tracker + inventory (crops)" on the two handles
alternates step by step, every step synchronised; medians with p10 / p90.  Both logs are drained after every pair of steps,
outside the timed regions, so no log fills and every closing's picture is moved.  The inventory launches' own time (the deciding
kernel and the picture launch with a store, the one kernel without) comes from events around lp_inventory_device.

"approaching": 6e's worst case, model-free.  Eight signs per frame grow from frame to frame, so every sighting is a new best;
consecutive calls carry other track ids, so every call also closes and logs the eight signs per stream of the call before.
Without a store the inventory copies a crop inline for every sighting (6e's figures); with a store the deciding kernel
copies the same crops and the picture launch moves only what survives the call: per stream and sign one gallery -> log
copy and one frame -> gallery picture.  Events around lp_inventory_device alone, the three shapes, no store / E 64 / E 128.

Seeded synthetic v1 detector whose class bias puts ~8 candidates per frame over conf 0.25 (bench.py's calibration), random
ShuffleNetV2 classifier, noise frames, as tools/inventory_bench.py.  Prints one JSON line.
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


def _alternate(fn_a, fn_b, steps, warmup, between):
    """between(): called after every pair of steps, outside the timed regions"""
    ta, tb = [], []
    for i in range(warmup + steps):
        for fn, acc in ((fn_a, ta), (fn_b, tb)):
            t0 = time.perf_counter()
            fn()
            if i >= warmup:
                acc.append((time.perf_counter() - t0) * 1e3)
        between()
    return _q(ta), _q(tb)


def approaching(e, st, torch, shapes, reps, sizes, frames):
    """model-free: 8 growing signs per frame, 64 frames per call, every record has a crop; two sets of ids alternate"""
    from litepi._ffi import DET_DTYPE, TRACK_DTYPE
    B, MD, K = 64, e.cfg.max_det, 8
    S = e.cfg.cls_input
    rng = np.random.default_rng(5)
    e.test_set_rois(rng.integers(0, 256, (B * K, S, S, 3), dtype=np.uint8), np.repeat(np.arange(B), K), np.tile(np.arange(K), B))
    e.test_set_frames(frames)
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
        out[name] = {}
        for E in (0,) + tuple(sizes):
            e.tracker_create(n_streams=B, max_tracks=64)
            e.inventory_create(max_signs=1 << 12, best="area")
            if E:
                e.evidence_create(size=E)
            ev = []
            pictures = 0
            for r in range(reps + 5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                e.inventory_device(dd.data_ptr(), dc.data_ptr(), bufs[r % 2].data_ptr(), B, sid, crops=True)
                e1.record(st)
                e.synchronize()
                if r >= 5:
                    ev.append(e0.elapsed_time(e1))
                if E:
                    signs = e.inventory_drain_evidence(crops=False)[0]
                    pictures = int((signs["flags"] & 4 != 0).sum())
                else:
                    signs = e.inventory_drain(crops=False)[0]
            out[name]["no_store" if not E else f"E{E}"] = dict(inventory_events=_q(ev), crops_copied_per_call=B * K,
                                                               signs_per_call=int(len(signs)), pictures_logged_per_call=pictures)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    import inventory_ref as V
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state

    tmp = tempfile.mkdtemp(prefix="evidence_bench_")
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
    e.close()
    st = torch.cuda.Stream()
    cls = random_shufflenet_state(NC, seed=3)
    engines = []
    for _ in range(2):   # [0]: no store, [1]: with a store
        g = Engine(precision="fp16", max_batch=B, max_det=MD, num_classes=NC)
        g.load_detector(p, b)
        g.load_classifier(cls)
        g.set_stream(st.cuda_stream)
        engines.append(g)
    bufs = [(torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda"), torch.zeros(3 * B, dtype=torch.int32, device="cuda"),
             torch.zeros(B * MD * 32, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    d_img = torch.from_numpy(imgs).cuda()
    torch.cuda.synchronize()
    tcfg = dict(n_streams=B, max_tracks=64)
    icfg = dict(max_signs=1 << 12, best=V.BEST_AREA)
    shapes = {"64x1": np.arange(B, dtype=np.int32), "8x8": np.repeat(np.arange(8, dtype=np.int32), 8), "1x64": np.zeros(B, np.int32)}
    sizes = (64, 128)
    res = dict(workload="64 x 640x640 frames, fp16, synthetic v1 detector + ShuffleNetV2, conf 0.25, max_det 300, max_tracks 64, "
                        "LP_BEST_AREA, keep_crops 1, max_signs 4096, evidence scale 2")

    def step(i, sid, timed=None):
        g, (dd, dc, dt) = engines[i], bufs[i]
        g.run_batch_device(d_img.data_ptr(), B, 640, 640, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
        g.track_device(dd.data_ptr(), dc.data_ptr(), B, dt.data_ptr(), sid)
        if timed is not None:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
        g.inventory_device(dd.data_ptr(), dc.data_ptr(), dt.data_ptr(), B, sid, crops=True)
        if timed is not None:
            e1.record(st)
        g.synchronize()
        if timed is not None:
            timed.append(e0.elapsed_time(e1))

    for E in sizes:
        for name, sid in shapes.items():
            for i, g in enumerate(engines):
                g.tracker_create(**tcfg)
                g.inventory_create(**icfg)
                if i:
                    g.evidence_create(size=E)
            tally = dict(signs=0, pictures=0, dropped=0, calls=0)

            def drain_both():   # after every pair of steps, untimed: the log never fills, every closing's picture is moved
                engines[0].inventory_drain(crops=False)
                signs, _, _, _, dropped = engines[1].inventory_drain_evidence(crops=False)
                tally["signs"] += len(signs)
                tally["pictures"] += int((signs["flags"] & 4 != 0).sum())
                tally["dropped"] += dropped
                tally["calls"] += 1

            t_plain, t_store = _alternate(lambda: step(0, sid), lambda: step(1, sid), a.steps, a.warmup, drain_both)
            ev = ([], [])
            for _ in range(50):
                step(0, sid, ev[0])
                step(1, sid, ev[1])
                drain_both()
            res[f"E{E}_{name}"] = dict(without_store=t_plain, with_store=t_store,
                                       added_ms=round(t_store["median_ms"] - t_plain["median_ms"], 4),
                                       inventory_events_without_store=_q(ev[0]), inventory_events_with_store=_q(ev[1]),
                                       signs_logged_per_call=round(tally["signs"] / tally["calls"], 1),
                                       pictures_logged_per_call=round(tally["pictures"] / tally["calls"], 1), dropped=tally["dropped"])
    res["approaching"] = approaching(engines[1], st, torch, shapes, 50, sizes, imgs)
    for g in engines:
        g.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
