#!/usr/bin/env python3
"""What taking decoder surfaces in place costs and buys.

    python tools/surface_bench.py [--steps 200] [--warmup 20] [--pitch-align 256] [--out profiles/surface_bench.json]

One process, the same frames on every side, the sides alternating step by step, every step synchronised; medians with the
10th / 90th percentiles.  Two workloads, 64 x 640^2 and 32 x 2048^2, fp16.  Every surface is an allocation of its own per
plane with the pitch rounded up to 256.

  (a) surfaces_nv12   lp_run_surfaces_device on the NV12 surfaces where they lie
  (b) floor           the same frames as ONE contiguous NV12 batch through lp_run_batch_device with lp_set_input_format
  (c) gather          what a user has to do without (a): 2 x B hipMemcpy2DAsync device-to-device into that batch, then (b)
  (d) surfaces_p010   (a) on P010 surfaces of the same frames

and the converters' own times from lp_profile_next (the launch's own events) in the same run: surfaces_to_bgr next to
nv12_to_bgr, the yardstick, on the same frames.  Seeded synthetic v1 detector calibrated like tools/nv12_bench.py, random
ShuffleNetV2 classifier.  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "yolo-litepi_amd"))
sys.path.insert(0, os.path.join(_ROOT, "tools"))

HBM_TBPS = 8.0   # MI355X HBM3E peak
CONF, IOU, MIN_AREA = 0.25, 0.45, 50


def _hip_runtime():
    """the HIP runtime this process already has loaded (torch's): a second copy would be a second runtime"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64" in line}
    if not paths:
        raise RuntimeError("no HIP runtime is loaded in this process")
    hip = C.CDLL(sorted(paths)[0])
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpy2DAsync.restype = C.c_int
    return hip


def _q(t):
    return dict(median_ms=round(float(np.median(t)), 4), p10_ms=round(float(np.percentile(t, 10)), 4),
                p90_ms=round(float(np.percentile(t, 90)), 4), steps=len(t))


def _alternate(sides, sync, steps, warmup):
    acc = {k: [] for k in sides}
    for i in range(warmup + steps):
        for k, fn in sides.items():
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= warmup:
                acc[k].append((time.perf_counter() - t0) * 1e3)
    return {k: _q(v) for k, v in acc.items()}


def _profiled(e, sides, reps):
    """per-launch times of the converters over `reps` profiled (eager) calls per side, the sides alternating"""
    acc = {}
    for _ in range(reps):
        for fn in sides.values():
            e.profile_next(True)
            fn()
            e.synchronize()
            for r in e.profile_read():
                if r["layer"] == "csc":
                    acc.setdefault(r["name"], []).append((r["ms"], r["bytes"]))
    out = {}
    for n, v in acc.items():
        ms = np.array([x[0] for x in v], np.float64)
        by = v[0][1]
        rate = lambda t: round(by / (t * 1e9), 3)   # noqa: E731
        out[n] = dict(median_ms=round(float(np.median(ms)), 5), p10_ms=round(float(np.percentile(ms, 10)), 5),
                      p90_ms=round(float(np.percentile(ms, 90)), 5), bytes=by, tb_per_s=rate(float(np.median(ms))),
                      tb_per_s_p10_p90=[rate(float(np.percentile(ms, 90))), rate(float(np.percentile(ms, 10)))],
                      hbm_fraction=round(by / (float(np.median(ms)) * 1e9) / HBM_TBPS, 3), launches=len(v))
    return out


def workload(torch, hip, p, b, cls_state, nv, steps, warmup, pitch_align=256):
    """nv: [B, H * 3 // 2, W] tight NV12 host frames"""
    from litepi import Engine
    from litepi.surfaces import surface_from_tensors
    B, H, W = nv.shape[0], nv.shape[1] // 3 * 2, nv.shape[2]
    e = Engine(precision="fp16", max_batch=B, max_det=300, num_classes=58)
    e.load_detector(p, b)
    e.load_classifier(cls_state)
    st = torch.cuda.Stream()
    e.set_stream(st.cuda_stream)
    dd = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
    dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    d_nv = torch.from_numpy(nv).cuda()                    # the floor's contiguous batch
    d_gather = torch.empty_like(d_nv)                     # (c) gathers into a batch of its own
    rng = torch.Generator(device="cuda").manual_seed(1)
    surf = {"nv12": [], "p010": []}
    keep = []
    for i in range(B):   # every plane its own allocation, pitch rounded up to 256 bytes
        for fmt, bps, dt in (("nv12", 1, torch.uint8), ("p010", 2, torch.int16)):
            pitch = -(-W * bps // pitch_align) * pitch_align
            y = torch.empty((H, pitch // bps), dtype=dt, device="cuda")[:, :W]
            uv = torch.empty((H // 2, pitch // bps), dtype=dt, device="cuda")[:, :W]
            src_y, src_uv = d_nv[i, :H], d_nv[i, H:]
            if fmt == "p010":   # value in the high byte, noise in the low byte
                lo = lambda s: torch.randint(0, 256, s.shape, generator=rng, device="cuda", dtype=torch.int32)   # noqa: E731
                y.copy_(((src_y.to(torch.int32) << 8) | lo(src_y)).to(torch.int16))
                uv.copy_(((src_uv.to(torch.int32) << 8) | lo(src_uv)).to(torch.int16))
            else:
                y.copy_(src_y)
                uv.copy_(src_uv)
            s, got = surface_from_tensors(y, uv)
            assert got == fmt and s.pitch_y == pitch
            surf[fmt].append(s)
            keep.append((y, uv))
    torch.cuda.synchronize()
    stream = C.c_void_p(st.cuda_stream)

    def floor(buf=d_nv):
        e.set_input_format("nv12")
        e.run_batch_device(buf.data_ptr(), B, H, W, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())

    def gather():
        fb = H * 3 // 2 * W
        for i, s in enumerate(surf["nv12"]):
            base = d_gather.data_ptr() + i * fb
            for dst, src, pitch, rows in ((base, s.y_ptr, s.pitch_y, H), (base + H * W, s.uv_ptr, s.pitch_uv, H // 2)):
                rc = hip.hipMemcpy2DAsync(dst, W, src, pitch, W, rows, 3, stream)   # 3 = hipMemcpyDeviceToDevice
                if rc != 0:
                    raise RuntimeError(f"hipMemcpy2DAsync returned {rc}")
        floor(d_gather)

    def surfaces(fmt):
        return lambda: e.run_surfaces_device(surf[fmt], CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr(), pixfmt=fmt)

    sides = {"surfaces_nv12": surfaces("nv12"), "floor_contiguous_nv12": floor, "gather_then_floor": gather, "surfaces_p010": surfaces("p010")}
    kept = {}
    for k, fn in sides.items():   # the four sides see the same pixels: the same counts
        fn(); e.synchronize()
        kept[k] = dc.cpu().numpy()[:B].copy()
    before = e.graph_stats()
    t = _alternate(sides, e.synchronize, steps, warmup)
    after = e.graph_stats()
    out = dict(frames=f"{B} x {W}x{H}", sides=t,
               same_counts=bool(all(np.array_equal(v, kept["floor_contiguous_nv12"]) for v in kept.values())),
               kept_total=int(kept["floor_contiguous_nv12"].sum()),
               surfaces_minus_floor_ms=round(t["surfaces_nv12"]["median_ms"] - t["floor_contiguous_nv12"]["median_ms"], 4),
               gather_minus_surfaces_ms=round(t["gather_then_floor"]["median_ms"] - t["surfaces_nv12"]["median_ms"], 4),
               p010_minus_nv12_ms=round(t["surfaces_p010"]["median_ms"] - t["surfaces_nv12"]["median_ms"], 4),
               graph_stats_delta={k: after[k] - before[k] for k in after})
    out["kernels"] = _profiled(e, {k: sides[k] for k in ("surfaces_nv12", "floor_contiguous_nv12", "surfaces_p010")}, 50)
    e.set_stream(0)
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pitch-align", type=int, default=256, help="every plane's pitch is its row rounded up to this (a multiple of 2)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from litepi import Engine, ncnn_export, synth
    from litepi.backend import random_shufflenet_state
    from nv12_bench import bgr_to_nv12

    hip = _hip_runtime()
    tmp = tempfile.mkdtemp(prefix="surface_bench_")
    p, b = os.path.join(tmp, "v1.param"), os.path.join(tmp, "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    rng = np.random.default_rng(7)
    nv = np.stack([bgr_to_nv12(rng.integers(0, 256, (640, 640, 3), dtype=np.uint8)) for _ in range(64)])
    e = Engine(precision="fp16", max_batch=16, max_det=300, num_classes=58)
    e.load_detector(p, b)
    s = np.sort(e.detect_raw(e.test_convert_frames(nv[:16], 16, 640, 640))[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    e.close()
    k = 8 * 16   # ~8 candidates per frame over conf 0.25 (bench.py's calibration)
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
    cls_state = random_shufflenet_state(58, seed=3)
    res = dict(workload="fp16, synthetic v1 detector + ShuffleNetV2, conf 0.25; every surface plane its own allocation, pitch rounded up to " + str(a.pitch_align))
    res["64x640"] = workload(torch, hip, p, b, cls_state, nv, a.steps, a.warmup, a.pitch_align)
    big = synth.config4_images(4, seed=2, size=2048, grain=8)
    four = [bgr_to_nv12(big[i]) for i in range(4)]
    res["32x2048"] = workload(torch, hip, p, b, cls_state, np.stack([four[i % 4] for i in range(32)]), a.steps, a.warmup, a.pitch_align)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
