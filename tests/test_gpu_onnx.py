"""GPU tests of the ONNX loader (lp_load_detector_onnx): an ONNX export reaches the plan of its NCNN twin.

Every comparison between an ONNX-loaded and an NCNN-loaded handle is equality -- out0 byte for byte, the profiled launches
(kernel name, flops, bytes) as sorted lists, pipeline records dict for dict: the reader lowers to the layers the NCNN export has
(tests/test_onnx_cpu.py), the planner is structural and the kernels are deterministic.  The one tolerance is DESIGN section 5's
fp32 out0 bound (score 1e-3, box abs + rel 1e-3), against the oracle's own ONNX interpreter (oracle/onnx_ref.py) reading the same
file: a second reading that shares no code with the loader or with tests/onnx_write.py.

The files: the reference's own export of the v1 checkpoint (oracle/_ref/yolo_plus_v1.onnx, staged by build() where the reference
is present; skipped otherwise) and ONNX files tests/onnx_write.py writes from seeded NCNN models, at the smallest sizes that
reach every plan: 320 x 320 with capacity 8 (the whole-C2f fp16 plan), 224 x 416 (rectangular), nc = 3, opset 17."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import onnx_write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = os.path.join(ROOT, "oracle", "_ref")
V1_PARAM, V1_BIN, V1_ONNX = (os.path.join(_REF, "yolo_plus_v1." + ext) for ext in ("param", "bin", "onnx"))
needs_v1_onnx = pytest.mark.skipif(not (os.path.exists(V1_PARAM) and os.path.exists(V1_BIN) and os.path.exists(V1_ONNX)),
                                   reason="reference v1 NCNN + ONNX exports not staged (build() stages them when the reference is present)")

pytestmark = pytest.mark.gpu


def _hw(size):
    return (size, size) if isinstance(size, int) else tuple(size)


def _images(size, B, seed):
    h, w = _hw(size)
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, 3), dtype=np.uint8)


def _observe(load, imgs, prec, cap, size):
    """out0 of `imgs` and the launches of that pass on a fresh handle whose detector `load(engine)` loads"""
    from litepi import Engine
    e = Engine(precision=prec, max_batch=cap, det_input=size)
    try:
        load(e)
        e.profile_next(True)
        out = e.detect_raw(imgs)
        prof = e.profile_read()
        launches = [(k["name"], k["flops"], k["bytes"]) for k in prof]
        _observe.layers = [k["layer"] for k in prof]
        info = (e.num_anchors, e.det_classes, e.reg_max, e.det_macs)
    finally:
        e.close()
    return out, launches, info


def _assert_twins(onnx_path, param, binf, prec, cap, size, B, seed=0):
    imgs = _images(size, B, seed)
    want, l_want, i_want = _observe(lambda e: e.load_detector(param, binf), imgs, prec, cap, size)
    got, l_got, i_got = _observe(lambda e: e.load_detector(onnx_path), imgs, prec, cap, size)   # one argument: lp_load_detector_onnx
    assert i_got == i_want
    assert len(l_got) == len(l_want) and sorted(l_got) == sorted(l_want), f"launches differ:\n{sorted(l_got)}\n{sorted(l_want)}"
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), f"out0 differs: max |d| {np.abs(got - want).max()}"
    assert np.isfinite(got).all() and float(got[:, 4:].max()) > 0.0
    return got, imgs, l_got


def _assert_oracle_bound(got, onnx_path, imgs):
    """score 1e-3, box abs + rel 1e-3 -- against oracle.onnx_ref on the same file"""
    from oracle import onnx_ref
    x = torch.from_numpy(imgs[..., ::-1].astype(np.float32) * np.float32(1 / 255.0)).permute(0, 3, 1, 2).contiguous()
    ref = np.concatenate([onnx_ref.forward(onnx_path, x[i:i + 1]).numpy() for i in range(len(imgs))])   # (the export is batch 1)
    assert got.shape == ref.shape
    err_b, err_s = np.abs(got[:, :4] - ref[:, :4]), np.abs(got[:, 4:] - ref[:, 4:])
    print(f"{os.path.basename(onnx_path)}: score err max {err_s.max():.2e}, box err max {err_b.max():.2e}")
    assert (err_b <= 1e-3 + 1e-3 * np.abs(ref[:, :4])).all(), f"box rows: max err {err_b.max()}"
    assert err_s.max() <= 1e-3, f"score rows: max err {err_s.max()}"


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    """(param, bin, onnx) of seeded synthetic detectors, written on first use"""
    from litepi import ncnn_export
    d = tmp_path_factory.mktemp("twins")
    made = {}

    def get(preset, size, nc=1, opset=12, cls_bias=-2.0):
        key = (preset, size, nc, opset, cls_bias)
        if key not in made:
            stem = str(d / f"{preset}_{'x'.join(map(str, _hw(size)))}_{nc}_{cls_bias}")
            if not os.path.exists(stem + ".param"):
                ncnn_export.export_detector(stem + ".param", stem + ".bin", preset, seed=77, nc=nc, size=size, cls_bias=cls_bias)
            onnx_write.ncnn_to_onnx(stem + ".param", stem + ".bin", f"{stem}_{opset}.onnx", size, opset=opset)
            made[key] = (stem + ".param", stem + ".bin", f"{stem}_{opset}.onnx")
        return made[key]
    return get


# ---- the reference's own export ---------------------------------------------------------------------------------------------------
@needs_v1_onnx
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_authentic_v1_same_bits_same_launches(prec):
    got, imgs, launches = _assert_twins(V1_ONNX, V1_PARAM, V1_BIN, prec, 2, 640, 2)
    assert got.shape == (2, 5, 8400) and len(launches) >= 10
    # layer names are the ONNX node names ("/model.0/conv/Conv+..."), cut to lp_kernel_time::layer's 31 characters
    layers = _observe.layers   # (of the ONNX-loaded handle: the second one observed)
    assert all(len(n) <= 31 for n in layers) and any(n.startswith("/model.") for n in layers) and max(map(len, layers)) == 31, layers
    if prec == "fp32":
        _assert_oracle_bound(got[:1], V1_ONNX, imgs[:1])


# ---- writer-made files --------------------------------------------------------------------------------------------------------------
def test_independent_reading_of_a_writer_made_file(twins):
    """fp32 out0 of the ONNX-loaded handle against oracle.onnx_ref on the same opset-12 file: loader and writer cannot agree on a
    wrong reading without the oracle's interpreter, which knows neither, disagreeing"""
    from litepi import Engine
    p, b, o = twins("v1", 320)
    imgs = _images(320, 1, 3)
    e = Engine(precision="fp32", max_batch=1, det_input=320)
    try:
        e.load_detector_onnx(o)
        got = e.detect_raw(imgs)
        # blob names are the ONNX tensor names: the first C2f's cv1 activation (the third conv), 16 channels at a quarter of the size
        assert e.debug_blob("/silu_2/Mul_output_0").shape == (1, 16, 80, 80)
    finally:
        e.close()
    _assert_oracle_bound(got, o, imgs)


@pytest.mark.parametrize("preset", ["v1", "v2"])
def test_whole_c2f_plan_320_batch3_fp16(twins, preset):
    p, b, o = twins(preset, 320)
    _, _, launches = _assert_twins(o, p, b, "fp16", 8, 320, 3)
    assert any(name.startswith("c2f") for name, _, _ in launches), [n for n, _, _ in launches]   # capacity 8: the whole-C2f plan is on


def test_rectangular_224x416_fp32_v2(twins):
    p, b, o = twins("v2", (224, 416))
    _assert_twins(o, p, b, "fp32", 2, (224, 416), 2)


def test_three_classes(twins):
    p, b, o = twins("v1", 320, nc=3)
    got, _, _ = _assert_twins(o, p, b, "fp16", 2, 320, 2)
    assert got.shape == (2, 7, 2100)


def test_opset17_forms(twins):
    p, b, o = twins("v2", 320, opset=17)
    _assert_twins(o, p, b, "fp16", 8, 320, 3)


def _param_at_320(src, dst):
    """the reference's YOLOv8n graph file is a 640 x 640 export: the same graph at 320 x 320 (a quarter of the anchors per level)"""
    out = []
    for ln in open(src):
        t = ln.split()
        if t and t[0] in ("MemoryData", "Reshape"):
            t = [f"{kv.split('=')[0]}={int(kv.split('=')[1]) // 4}" if "=" in kv and kv.split("=")[1] in ("8400", "6400", "1600", "400") else kv for kv in t]
            ln = " ".join(t) + "\n"
        out.append(ln)
    with open(dst, "w") as f:
        f.writelines(out)


def test_yolov8n_graph_seeded_320(tmp_path):
    from litepi import ncnn_export
    src = os.path.join(_REF, "yolo8_tt100k.param")
    if not os.path.exists(src):
        pytest.skip("reference graph files not staged (build() stages them when the reference is present)")
    p, b, o = str(tmp_path / "y8.param"), str(tmp_path / "y8.bin"), str(tmp_path / "y8.onnx")
    _param_at_320(src, p)
    ncnn_export.seeded_bin_for_param(p, b, seed=5, size=320)
    info = onnx_write.ncnn_to_onnx(p, b, o, 320)
    assert info["num_anchors"] == 2100
    _assert_twins(o, p, b, "fp16", 4, 320, 2)


# ---- handle behaviour -----------------------------------------------------------------------------------------------------------------
def test_onnx_load_replaces_model_and_drops_captured_graphs(twins):
    """a handle that holds an NCNN model and a captured lp_run_batch_device step loads an ONNX model: the next call of the same
    key gives the new model's records"""
    from litepi import Engine
    from litepi._ffi import DET_DTYPE
    from litepi.backend import random_shufflenet_state
    from litepi.distributed import alloc_result_buffers
    pa, ba, _ = twins("v1", 320, cls_bias=1.5)
    pb, bb, ob = twins("v2", 320, cls_bias=1.5)
    B, dev = 2, torch.device("cuda", 0)
    imgs = _images(320, B, 5)
    cls_state = random_shufflenet_state(91, seed=3)
    eng, ref = (Engine(precision="fp16", max_batch=B, max_det=50, num_classes=91, det_input=320) for _ in range(2))
    try:
        for e, (p, b) in ((eng, (pa, ba)), (ref, (pb, bb))):
            e.load_detector(p, b)
            e.load_classifier(cls_state)
        want_a = eng.run_batch(list(imgs), 0.25, 0.45, 0)
        want_b = ref.run_batch(list(imgs), 0.25, 0.45, 0)
        assert int(want_a[1].sum()) > 0 and int(want_b[1].sum()) > 0
        assert want_a[0].tobytes() != want_b[0].tobytes()
        dimg = torch.from_numpy(imgs).to(dev)
        res = alloc_result_buffers(B, 50, dev)
        st = torch.cuda.Stream(device=dev)
        eng.set_stream(st.cuda_stream)

        def step():
            with torch.cuda.stream(st):
                eng.run_batch_device(dimg.data_ptr(), B, 320, 320, 0.25, 0.45, 0, res.dets.data_ptr(), res.counts.data_ptr())
                eng.synchronize()
            torch.cuda.synchronize()
            counts = res.counts.cpu().numpy()[:B].astype(np.int64)
            recs = res.dets.cpu().numpy().reshape(B, -1).view(DET_DTYPE).reshape(B, -1)
            return counts, [recs[i, :counts[i]].tobytes() for i in range(B)]

        def records(want):
            return [want[0][i, :want[1][i]].tobytes() for i in range(B)]

        for call in range(3):   # eager, capture, replay
            counts, recs = step()
            assert np.array_equal(counts, want_a[1]) and recs == records(want_a), f"model A, call {call}"
        eng.load_detector_onnx(ob)
        for call in range(3):
            counts, recs = step()
            assert np.array_equal(counts, want_b[1]) and recs == records(want_b), f"model B from ONNX, call {call}"
    finally:
        eng.close()
        ref.close()


def test_wrong_size_export_is_refused_and_memory_form(twins):
    from litepi import Engine, _ffi
    p640, b640, o640 = twins("v1", 640)
    _, _, o320 = twins("v1", 320)
    imgs = _images(640, 1, 9)
    e = Engine(precision="fp16", max_batch=1)
    try:
        e.load_detector(p640, b640)
        before = e.detect_raw(imgs)
        with pytest.raises(_ffi.LitepiError) as ei:
            e.load_detector_onnx(o320)   # a 320 x 320 export on a 640 x 640 handle
        assert ei.value.code == _ffi.LP_ERR_GRAPH, str(ei.value)
        assert e.detect_raw(imgs).tobytes() == before.tobytes()   # the old model still answers
        with pytest.raises(_ffi.LitepiError) as ei:
            e.load_detector_onnx(o640 + ".missing")
        assert ei.value.code == _ffi.LP_ERR_IO
        e.load_detector_onnx(o640)
        from_path = e.detect_raw(imgs)
        assert from_path.tobytes() == before.tobytes()
        with open(o640, "rb") as f:
            e.load_detector_onnx(f.read())   # lp_load_detector_onnx_memory
        assert e.detect_raw(imgs).tobytes() == from_path.tobytes()
    finally:
        e.close()


# ---- front to back ------------------------------------------------------------------------------------------------------------------
def _strip(results):
    """the records of a run_batch call without their timings, as plain Python values"""
    return [[{k: np.asarray(v).tolist() for k, v in r.items() if k not in ("time_det", "time_cls")} for r in res] for res, _ in results]


def test_hybrid_pipeline_from_onnx_file(twins, tmp_path):
    from litepi import HybridPipeline
    from oracle import shufflenet_ref as S
    p, b, o = twins("v1", 320, cls_bias=1.5)
    cls_path = str(tmp_path / "cls.pth")
    torch.save(S.seeded_state_dict(91), cls_path)
    frames = list(np.random.default_rng(21).integers(0, 256, (2, 240, 320, 3), dtype=np.uint8))
    outs = []
    for det in ((p, b), (o, None)):
        pipe = HybridPipeline(det[0], det[1], cls_path, "shufflenetv2", num_classes=91, det_input_size=320, precision="fp16", max_batch=2,
                              max_det=50, track=True)
        try:
            outs.append([_strip(pipe.run_batch(frames, 0.25, 0.45, 0)) for _ in range(2)])   # two calls: the tracker sees a sequence
        finally:
            pipe.close()
    assert sum(len(r) for r in outs[0][0]) > 0 and "track_id" in outs[0][1][0][0]
    assert outs[0] == outs[1]


def test_e2e_cli_detector_onnx_in_a_child_process(twins, tmp_path):
    import json
    import pandas as pd
    from PIL import Image
    from litepi import e2e
    from oracle import shufflenet_ref as S
    p, b, o = twins("v1", 320, cls_bias=1.5)
    ncls = 5
    rng = np.random.default_rng(31)
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir(); lab_dir.mkdir()
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(img_dir / f"im{i}.png")
        (lab_dir / f"im{i}.txt").write_text(f"{i} 0.5 0.5 0.2 0.2\n")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(ncls)}))
    cls_path = str(tmp_path / "cls.pth")
    torch.save(S.seeded_state_dict(ncls), cls_path)
    common = ["--classifier", cls_path, "--clf_arch", "shufflenetv2", "--input", str(img_dir), "--labels", str(lab_dir), "--classes", str(classes),
              "--det_input_size", "320", "--batch_images", "2", "--max_det", "50"]
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "yolo-litepi_amd"), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "litepi.e2e", "--detector_onnx", o, "--output", str(tmp_path / "out_onnx")] + common, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert e2e.main(["--detector_param", p, "--detector_bin", b, "--output", str(tmp_path / "out_ncnn")] + common) == 0
    rows = [pd.read_csv(tmp_path / d / "comparison_summary.csv") for d in ("out_onnx", "out_ncnn")]
    same = ["classifier", "num_test_images", "mean_precision", "mean_recall", "mean_f1", "mAP50", "mAP50-95"]   # (not the names, not the fps)
    assert len(rows[0]) == len(rows[1]) == 1 and rows[0].loc[0, "num_test_images"] == 2
    assert rows[0][same].equals(rows[1][same]), f"{rows[0][same]}\n{rows[1][same]}"
    assert rows[0].loc[0, "detector"] != rows[1].loc[0, "detector"]
