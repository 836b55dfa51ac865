#!/usr/bin/env python3
"""Phase stamps of the fused Detect-head kernel (diagnostic; GPU box): LITEPI_HEAD_STAMPS=<file> makes every head launch dump
16 clock stamps per workgroup; this runs a warm batch-64 detect and prints, per level, the share of workgroups that left at the vote (no
anchor of their tile can pass conf) and per-phase cycle statistics of those that stayed and of those that left.

    python tools/head_stamps.py [v1|v2] [raw|bench]

"bench": bench.py's first batch and its detector, calibrated as bench.py calibrates it (~8 anchors per image above conf 0.25)."""
import os, sys, tempfile
import numpy as np
path = os.path.join(tempfile.mkdtemp(), "stamps.bin")
os.environ["LITEPI_HEAD_STAMPS"] = path
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "yolo-litepi_amd"))
from litepi import Engine, ncnn_export  # noqa: E402
d = tempfile.mkdtemp()
p, b = os.path.join(d, "m.param"), os.path.join(d, "m.bin")
mode = sys.argv[2] if len(sys.argv) > 2 else ""
B = 64
# "bench": bench.py's first batch (its calibration images are the first eight of it)
imgs = np.random.default_rng(1 if mode == "bench" else 0).integers(0, 256, (B, 640, 640, 3), dtype=np.uint8)
ncnn_export.export_detector(p, b, sys.argv[1] if len(sys.argv) > 1 else "v1", seed=1234, cls_bias=0.0 if mode == "bench" else -4.0)
if mode == "bench":   # bench.py:build_models: the k-th best score of the engine's own out0 on 8 images goes to conf
    e = Engine(precision="fp16", max_batch=B)
    e.load_detector(p, b)
    s = np.sort(e.detect_raw(imgs[:8])[:, 4].astype(np.float64).ravel())[::-1]
    e.close()
    kth = min(max(s[8 * 8], 1e-6), 1 - 1e-6)
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - np.log(kth / (1 - kth))))
e = Engine(precision="fp16", max_batch=B)
e.load_detector(p, b)
# "raw": the parity hook (every anchor decoded, out0 written); default: the product path (conf filter, decode only where needed)
raw_path = mode == "raw"
os.environ["LITEPI_NO_GRAPH"] = "1"
run = (lambda: e.detect_raw(imgs)) if raw_path else (lambda: e.detect(list(imgs), 0.25, 0.45))
run()
open(path, "wb").close()          # keep only the second (warm) call
run()
e.close()
raw = np.fromfile(path, dtype=np.uint64)
# stamps 2..9 (cycles, each minus the one before): a workgroup that leaves at the vote writes 2..7 only; stamp 14 = 1 marks it.
# Split stage A (the v1 default shapes): stage A in front of the vote is the class tower's first conv alone, and a workgroup that
# stays runs the box tower's behind the vote -- stamps 10..13, in time between 7 and 8: box pass entered, its K loops done (the hand-off
# and, where MID overlays the input tile, the tile's second staging are inside), its SiLU epilogue entered (behind the overlay barrier)
# and done.  They are zero in a leaver and on the shapes with the merged stage A (v2, LITEPI_HEAD_MERGED_A=1, the 32-pixel-slot shapes).
names = {2: "issued", 3: "chunk0 landed", 4: "stage A loop", 5: "A epilogue", 6: "B cls", 7: "cls proj + vote", 10: "(box pass entered)",
         11: "A box: tile + loop", 12: "A box: barrier", 13: "A box epilogue", 8: "B box", 9: "box proj + decode"}
off = 0
while off < len(raw):
    assert raw[off] == 0x48454144
    grid, H, N = int(raw[off + 1]), int(raw[off + 2]), int(raw[off + 3])
    s = raw[off + 4: off + 4 + grid * 16].reshape(grid, 16).astype(np.int64)
    off += 4 + grid * 16
    wall = (s[:, 15] - s[:, 0])            # 100 MHz ticks
    left = s[:, 14] == 1
    print(f"level {H}x{H}: {grid} workgroups, {int(left.sum())} left at the vote ({100.0 * left.mean():.1f} %); "
          f"kernel span {(s[:, 15].max() - s[:, 0].min()) / 100:.1f} us")
    split_a = bool((s[~left][:, 10:14] != 0).all()) if (~left).any() else False
    stay_order = [2, 3, 4, 5, 6, 7] + ([10, 11, 12, 13] if split_a else []) + [8, 9]
    for tag, sel, order in (("stayed" + (" (split stage A)" if split_a else ""), ~left, stay_order), ("left at the vote", left, [2, 3, 4, 5, 6, 7])):
        if not sel.any():
            continue
        q = s[sel]
        print(f"  {tag}: {int(sel.sum())} workgroups, per-WG wall {np.median(wall[sel]) / 100:.2f} us median, "
              f"{np.median(q[:, order[-1]] - q[:, 1]):.0f} cycles from start to the last stamp")
        prev = 1
        for k in order:
            dt = q[:, k] - q[:, prev]
            print(f"   {names[k]:18s} median {np.median(dt):9.0f} cyc   p90 {np.percentile(dt, 90):9.0f}")
            prev = k
