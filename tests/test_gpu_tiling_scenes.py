"""GPU tests of tiled inference, second part (first part: test_gpu_tiling.py, groups 1-3, 5, 6):
  * the view gather itself against NumPy slices: unaligned source runs (odd frame widths, odd byte offsets) and the 114 fill
    of a frame narrower than det_input, on the host and the device path;
  * 4. fp16 at capacity 64, v1 and v2, scored against the CPU tiling oracle's confident boxes (configs[4] analogue);
  * 7. the CLI's --tile_overlap: the harness's predictions equal HybridPipeline.run_batch with the same tiling;
  * 8. the reference's real v1 weights on 2048x2048 scenes of the real sign crops: fp32 tiled equals the tiling oracle at
    conf 0.25 and 0.001; letterbox-vs-tiled sign counts are printed, not asserted."""
import io
import json
import os

import numpy as np
import pytest
import torch

import tiling_ref as T
from test_gpu_tiling import _calibrate_on_views

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REAL = (os.path.join(_ROOT, "oracle", "_ref", "yolo_plus_v1.param"), os.path.join(_ROOT, "oracle", "_ref", "yolo_plus_v1.bin"))


def _frame(rng, H, W):
    low = rng.integers(0, 256, (H // 16 + 1, W // 16 + 1, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(low, 16, 0), 16, 1)[:H, :W]
    return np.ascontiguousarray(img ^ rng.integers(0, 8, (H, W, 3), dtype=np.uint8))


# ---------------------------------------------------------------------------- the view gather against NumPy slices
@pytest.mark.parametrize("H,W", [(681, 1198), (2000, 500), (500, 2000), (1001, 1333), (2048, 2048)])
@pytest.mark.parametrize("offset", [0, 5])
def test_view_gather_matches_numpy(H, W, offset):
    from litepi import Engine
    rng = np.random.default_rng(H * 7 + W + offset)
    img = _frame(rng, H, W)
    e = Engine(precision="fp16", max_batch=32)
    try:
        got = e.test_tile_views(img, 128, True, offset)
        want = T.make_views(img, 640, 128, True)
        assert len(got) == len(want)
        for k, ((x, y, _, _), (v, _, _)) in enumerate(zip(T.tile_grid(640, H, W, 128, True), want)):
            if x < 0:   # the letterboxed whole frame: exactly lp_test_letterbox's bytes
                assert np.array_equal(got[k], e.test_letterbox(img)[0]), f"view {k} (letterbox)"
            else:
                assert np.array_equal(got[k], v), f"view {k} at ({x}, {y})"
        if W < 640 or H < 640:
            assert (got[1:] == 114).any(), "a frame narrower than det_input must show the 114 fill"
    finally:
        e.close()


def test_device_path_unaligned_frames_equal_host_path(tmp_path):
    """lp_run_tiled_device on frames whose rows are not 16-byte multiples, in a buffer at an odd byte offset, against lp_run_tiled"""
    from litepi import Engine, ncnn_export
    from litepi._ffi import DET_DTYPE
    from litepi.backend import random_shufflenet_state
    p, b = str(tmp_path / "m.param"), str(tmp_path / "m.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    rng = np.random.default_rng(4)
    frames = np.stack([_frame(rng, 681, 1198), _frame(rng, 681, 1198)])
    _calibrate_on_views(p, b, list(frames), 4, 8)
    e = Engine(precision="fp32", max_batch=16, max_det=300, num_classes=91)
    try:
        e.load_detector(p, b)
        e.load_classifier(random_shufflenet_state(91, seed=3))
        B = 2
        dets_ref, counts_ref, num_ref, _ = e.run_tiled(list(frames), 0.25, 0.45, 50)
        raw = torch.zeros(frames.nbytes + 64, dtype=torch.uint8, device="cuda")
        raw[5:5 + frames.nbytes] = torch.from_numpy(frames.reshape(-1)).cuda()
        dd = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for call in range(3):
            e.run_tiled_device(raw.data_ptr() + 5, B, 681, 1198, 0.25, 0.45, 50, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            cnt = dc.cpu().numpy()
            assert np.array_equal(cnt[:B], counts_ref) and np.array_equal(cnt[B:2 * B], num_ref), f"call {call}"
            recs = dd.cpu().numpy().view(DET_DTYPE).reshape(B, -1)
            for i in range(B):
                assert recs[i, :counts_ref[i]].tobytes() == dets_ref[i, :counts_ref[i]].tobytes(), f"call {call} frame {i}"
        assert int(num_ref.sum()) >= 1
    finally:
        e.close()


# ---------------------------------------------------------------------------- 4. fp16 at capacity 64, v1 and v2
def _box_iou(a, b):
    iw = max(0.0, min(a[2], b[2]) - max(a[0], b[0])); ih = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    u = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - iw * ih
    return iw * ih / u if u > 0 else 0.0


@pytest.mark.parametrize("preset", ["v1", "v2"])
def test_tiled_fp16_capacity64_map_vs_cpu(tmp_path, preset):
    """configs[4] tiled: three 2048x2048 frames (51 views) on a 64-view fp16 handle.  The CPU tiling oracle's confident boxes are
    pseudo ground truth; bounds of test_config4_large_images_map_vs_cpu."""
    from litepi import HybridPipeline, ncnn_export
    from litepi.e2e import evaluate_predictions
    from litepi.synth import config4_images
    from oracle import ncnn_ref, shufflenet_ref as S
    p, b = str(tmp_path / "m.param"), str(tmp_path / "m.bin")
    ncnn_export.export_detector(p, b, preset, seed=77, cls_bias=0.0)
    imgs = list(config4_images(3, seed=2, grain=8))
    if preset == "v2":   # v2's random class logits on these frames reach ~50: hundreds of scores per view are exactly 1.0 in fp32, so
        ncnn_export.shift_cls_bias(p, b, -30.0)   # the calibration (logit space) starts from a shifted bias and a deeper rank
        _calibrate_on_views(p, b, imgs, 60, 120)
    else:
        _calibrate_on_views(p, b, imgs, 10, 20)
    sd = S.seeded_state_dict(91)
    cpu = T.CpuTiledPipeline(ncnn_ref.load_model(p, b), S.build(91, sd))
    cls_path = str(tmp_path / "cls.pth")
    torch.save(sd, cls_path)
    pipe = HybridPipeline(p, b, cls_path, "shufflenetv2", num_classes=91, precision="fp16", max_batch=64, max_det=300,
                          tile_overlap=128, tile_full_frame=True)
    try:
        outs = pipe.run_batch(imgs, 0.25, 0.45, 50)
    finally:
        pipe.engine.close()
    all_preds, all_gts, found, total = [], [], 0, 0
    for im, (res, _m) in zip(imgs, outs):
        exp, _ = cpu.run(im, 0.25, 0.45, 50)
        strong = [x for x in exp if x["det_conf"] > 0.27 and x["cls_class"] >= 0]
        all_gts.append([(x["cls_class"],) + tuple(x["bbox"]) for x in strong])
        all_preds.append([{"bbox": r["bbox"], "conf": r["det_conf"], "cls_class": r["cls_class"]} for r in res])
        for x in strong:
            found += max([_box_iou(np.array(x["bbox"], np.float64), np.array(r["bbox"], np.float64)) for r in res] + [0.0]) >= 0.5
            total += 1
    assert total >= 6, "calibration produced too few confident detections"
    m = evaluate_predictions(all_preds, all_gts, 91)
    print(f"tiled config4 {preset}: {found}/{total} confident CPU boxes found; mAP50 {m['mAP50']:.3f} mAP50-95 {m['mAP50_95']:.3f}")
    assert found >= total - max(1, total // 24)
    assert m["mAP50"] >= 0.6 and m["mAP50_95"] >= 0.4


# ---------------------------------------------------------------------------- 7. CLI
def test_cli_tile_overlap_equals_run_batch(tmp_path):
    from PIL import Image
    from litepi import HybridPipeline, e2e, ncnn_export
    from litepi.synth import config4_images
    from oracle import shufflenet_ref as S
    import pandas as pd
    p, b = str(tmp_path / "synthetic.param"), str(tmp_path / "synthetic.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    imgs = list(config4_images(2, seed=9, grain=8))
    _calibrate_on_views(p, b, imgs, 4, 8)
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir(); lab_dir.mkdir()
    rng = np.random.default_rng(3)
    for i, im in enumerate(imgs):
        Image.fromarray(im[:, :, ::-1]).save(img_dir / f"f{i}.png")
        with open(lab_dir / f"f{i}.txt", "w") as f:
            for _ in range(3):
                f.write(f"{int(rng.integers(0, 91))} {rng.uniform(0.2, 0.8):.6f} {rng.uniform(0.2, 0.8):.6f} 0.020000 0.020000\n")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(91)}))
    cls_path = str(tmp_path / "cls.pth")
    torch.save(S.seeded_state_dict(91), cls_path)
    out = tmp_path / "out"
    argv = ["--detector_param", p, "--detector_bin", b, "--classifier", cls_path, "--input", str(img_dir), "--labels", str(lab_dir),
            "--classes", str(classes), "--output", str(out), "--yolo_conf", "0.1", "--max_det", "300", "--tile_overlap", "128"]
    assert e2e.main(argv) == 0
    df = pd.read_csv(out / "comparison_summary.csv")
    assert len(df) == 1 and df.loc[0, "num_test_images"] == 2
    r = e2e.run_evaluation(e2e.build_parser().parse_args(argv))
    pipe = HybridPipeline(p, b, cls_path, "shufflenetv2", num_classes=91, precision="fp16", max_batch=17, max_det=300, max_rois=300,
                          tile_overlap=128, tile_full_frame=True)
    try:
        want = [pipe.run_batch([im], 0.1, 0.45, 50)[0][0] for im in imgs]
    finally:
        pipe.engine.close()
    got = r["all_preds"]
    assert sum(len(g) for g in got) >= 2, "the calibrated model found nothing: the comparison is empty"
    for g, w in zip(got, want):
        assert [(x["bbox"], x["conf"], x["cls_class"]) for x in g] == [(x["bbox"], x["det_conf"], x["cls_class"]) for x in w]
    assert abs(df.loc[0, "mAP50"] - r["metrics"]["mAP50"]) < 1e-9


# ---------------------------------------------------------------------------- 8. real v1 weights
def _sign_scene():
    """the 15 debug ROIs pasted at native size on a smooth 2048x2048 background; returns the scene and the pasted rectangles"""
    from PIL import Image
    with np.load(os.path.join(_ROOT, "tests", "golden", "debug_rois.npz")) as z:
        crops = [np.asarray(Image.open(io.BytesIO(z[k].tobytes())).convert("RGB"))[..., ::-1].copy() for k in sorted(z.files)]
    rng = np.random.default_rng(2048)
    low = rng.integers(90, 160, (8, 8, 3)).astype(np.uint8)
    img = np.asarray(Image.fromarray(low).resize((2048, 2048), Image.BICUBIC)).copy()
    rects = []
    for k, c in enumerate(crops):
        gx, gy = k % 4, k // 4
        x, y = 100 + gx * 480 + int(rng.integers(0, 200)), 100 + gy * 480 + int(rng.integers(0, 200))
        h, w = c.shape[:2]
        img[y:y + h, x:x + w] = c
        rects.append((x, y, x + w, y + h))
    return img, rects


@pytest.mark.skipif(not all(os.path.exists(p) for p in _REAL), reason="the reference's v1 model is not staged under oracle/_ref")
def test_real_v1_weights_tiled_vs_oracle():
    from litepi import HybridPipeline
    from oracle import ncnn_ref, shufflenet_ref as S
    img, rects = _sign_scene()
    sd = S.seeded_state_dict(58)
    import tempfile
    cls_path = os.path.join(tempfile.mkdtemp(prefix="litepi_tiling_"), "cls.pth")
    torch.save(sd, cls_path)
    cpu = T.CpuTiledPipeline(ncnn_ref.load_model(*_REAL), S.build(58, sd))
    found = {}
    for mode in ("letterbox", "tiled"):
        pipe = HybridPipeline(*_REAL, cls_path, "shufflenetv2", num_classes=58, precision="fp32", max_batch=17, max_det=8400,
                              max_rois=8400, tile_overlap=128 if mode == "tiled" else None)
        try:
            for conf in (0.25, 0.001):
                res, met = pipe.run_batch([img], conf, 0.45, 50)[0]
                if mode == "tiled":
                    exp, exp_num = cpu.run(img, conf, 0.45, 50, overlap=128, full_frame=True)
                    assert met.num_detections == exp_num, f"conf {conf}: num_det {met.num_detections} vs oracle {exp_num}"
                    assert len(res) == len(exp), f"conf {conf}: {len(res)} results vs oracle {len(exp)}"
                    for r, x in zip(res, exp):
                        assert abs(r["det_conf"] - x["det_conf"]) <= 1e-3
                        assert np.abs(np.array(r["bbox"]) - np.array(x["bbox"])).max() <= 1
                        assert r["det_class"] == x["det_class"] and r["cls_class"] == x["cls_class"]
                    if conf == 0.001:
                        assert exp_num >= 50, f"only {exp_num} boxes at conf 0.001: the merge sees too little"
                if conf == 0.25:
                    found[mode] = sum(any(_box_iou(np.array(rc, np.float64), np.array(r["bbox"], np.float64)) >= 0.5 for r in res)
                                      for rc in rects)
        finally:
            pipe.engine.close()
    # a statement about the model, not asserted
    print(f"\n[tiling] real v1 weights, 2048x2048 scene of {len(rects)} pasted signs (10-84 px), conf 0.25, IoU >= 0.5: "
          f"letterbox finds {found['letterbox']}, tiled (overlap 128, full frame) finds {found['tiled']}")
