"""CPU suite (-m "not gpu"), part 1: the oracle is pinned.

* post-processing restatement == outputs of the REFERENCE's own functions (goldens made by
  tools/make_goldens.py in the build container), bit for bit;
* PIL-resize restatement == Pillow itself;
* NCNN reader extracts exactly the tensors the ONNX export of the same checkpoint holds;
* the oracle's forward on the real v1 weights is stable against committed checksums.

The reference's v1 checkpoint (NCNN + ONNX, 4 MB each) is too large to commit: __graft_entry__.build() stages it under
oracle/_ref/ where the reference checkout exists, and the tests that read it skip where it was not staged.
"""
import json
import os

import numpy as np
import pytest

_REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
V1_PARAM, V1_BIN, V1_ONNX = (os.path.join(_REF, "yolo_plus_v1." + ext) for ext in ("param", "bin", "onnx"))
needs_v1 = pytest.mark.skipif(not (os.path.exists(V1_PARAM) and os.path.exists(V1_BIN)),
                              reason="the reference's v1 model is not staged under oracle/_ref (build() without the reference)")
needs_v1_onnx = pytest.mark.skipif(not (os.path.exists(V1_PARAM) and os.path.exists(V1_BIN) and os.path.exists(V1_ONNX)),
                                   reason="the reference's v1 model + ONNX export are not staged under oracle/_ref")


def test_nms_matches_reference_goldens(golden_dir):
    from oracle import postprocess_ref as P
    g = np.load(os.path.join(golden_dir, "ref_nms.npz"))
    keys = [k[:-5] for k in g.files if k.endswith("_keep")]
    assert len(keys) == 11
    for k in keys:
        keep = P.nms(g[k + "_boxes"], g[k + "_scores"], float(g[k + "_thr"]))
        assert np.array_equal(keep, g[k + "_keep"]), k


def test_postprocess_matches_reference_goldens(postprocess_goldens):
    from oracle import postprocess_ref as P
    g = postprocess_goldens
    i = 0
    while f"c{i}_out0" in g:
        oh, ow, r, p0, p1, conf, iou = g[f"c{i}_geom"]
        b, s, c = P.postprocess(g[f"c{i}_out0"], (int(oh), int(ow)), r, (p0, p1), conf, iou)
        eb = g[f"c{i}_boxes"]
        assert b.shape == eb.shape and b.dtype == eb.dtype  # float64 empties included (e2e.py:264)
        assert np.array_equal(b, eb) and np.array_equal(s, g[f"c{i}_scores"]) and np.array_equal(c, g[f"c{i}_cls"])
        assert c.dtype == g[f"c{i}_cls"].dtype
        i += 1
    assert i == 8


def test_roi_logic_matches_reference_goldens(golden_dir):
    from oracle import postprocess_ref as P
    g = np.load(os.path.join(golden_dir, "ref_pipeline.npz"))
    for i in range(4):
        h, w, ma = g[f"c{i}_hw_minarea"]
        rects, valid = P.roi_rects(g[f"c{i}_boxes"], h, w, ma)
        shp = g[f"c{i}_roi_shapes"]
        assert np.array_equal(rects[:, 3] - rects[:, 1], shp[:, 0]) and np.array_equal(rects[:, 2] - rects[:, 0], shp[:, 1])
        assert np.array_equal(g[f"c{i}_boxes"][valid].astype(int), g[f"c{i}_res_bbox"])
        assert int(g[f"c{i}_num_detections"]) == len(g[f"c{i}_boxes"])


def test_letterbox_geometry_and_identity():
    from oracle import postprocess_ref as P
    r, unpad, (dw, dh), (t, b, l, rr) = P.letterbox_params(681, 1198)
    assert unpad == (640, 364) and (dw, dh) == (0.0, 138.0) and (t, b, l, rr) == (138, 138, 0, 0)
    r, unpad, (dw, dh), (t, b, l, rr) = P.letterbox_params(640, 359)   # odd padding: extra pixel right/bottom
    assert unpad == (359, 640) and dw == 140.5 and (l, rr) == (140, 141)
    img = np.random.default_rng(0).integers(0, 256, (640, 640, 3), dtype=np.uint8)
    out, r, pad = P.letterbox(img)
    assert np.array_equal(out, img) and r == 1.0 and pad == (0.0, 0.0)
    img = np.random.default_rng(0).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    out, r, pad = P.letterbox(img)
    assert out.shape == (640, 640, 3) and np.array_equal(out[80:560], img) and (out[:80] == 114).all() and (out[560:] == 114).all()


def test_pil_resize_restatement_equals_pillow():
    from PIL import Image
    from oracle import pil_resize_ref as R
    rng = np.random.default_rng(0)
    for (h, w) in [(10, 10), (7, 200), (200, 7), (64, 64), (64, 30), (30, 64), (1, 1), (2, 3), (129, 257), (63, 65), (300, 500)]:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.array(Image.fromarray(im).resize((64, 64), Image.BILINEAR))
        assert np.array_equal(R.resize_bilinear_u8(im, 64, 64), ref), (h, w)


def test_pil_resize_on_reference_debug_rois(golden_dir):
    """The 15 sign crops the reference keeps next to its pipeline (src/vntsr/pipeline/debug_rois), committed as the
    files' bytes."""
    import io
    from PIL import Image
    from oracle import pil_resize_ref as R
    with np.load(os.path.join(golden_dir, "debug_rois.npz")) as z:
        files = {k: z[k].tobytes() for k in z.files}
    assert len(files) == 15
    for name, data in sorted(files.items()):
        im = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
        ref = np.array(Image.fromarray(im).resize((64, 64), Image.BILINEAR))
        assert np.array_equal(R.resize_bilinear_u8(im, 64, 64), ref), name


@needs_v1_onnx
def test_ncnn_reader_matches_onnx_initializers():
    from oracle import ncnn_ref, onnx_init
    layers = ncnn_ref.load_model(V1_PARAM, V1_BIN)
    init = onnx_init.read_initializers(V1_ONNX)
    pool = [v for v in init.values() if v.dtype == np.float32]
    convs = ncnn_ref.conv_layers(layers)
    assert len(convs) == 64
    for l in convs:
        assert any(v.shape == l.weight.shape and np.array_equal(v, l.weight) for v in pool), l.name
        if l.bias is not None:
            assert any(v.shape == l.bias.shape and np.array_equal(v, l.bias) for v in pool), l.name
    assert ncnn_ref.conv_macs(layers) == 1418713600  # 1.4187 GMAC


@needs_v1
def test_oracle_forward_on_real_weights_is_stable(golden_dir):
    """Seeded rand(1,3,640,640) as in the reference's model_ncnn.py:6-7.  The reference holds no
    expected output (parity unpinned); this pins the oracle against silent drift only."""
    import torch
    from oracle import ncnn_ref
    layers = ncnn_ref.load_model(V1_PARAM, V1_BIN)
    g = np.load(os.path.join(golden_dir, "oracle_v1_out0_checksums.npz"))
    for seed in (0, 1):
        torch.manual_seed(seed)
        out = ncnn_ref.run_graph(layers, torch.rand(1, 3, 640, 640))["out0"].numpy()[0]
        assert out.shape == (5, 8400)
        assert np.allclose(out[:, ::97], g[f"s{seed}_sub"], rtol=1e-4, atol=1e-4)
        assert np.allclose(out.mean(axis=1), g[f"s{seed}_mean"], rtol=1e-4)


@needs_v1_onnx
def test_two_reference_graph_descriptions_agree_on_real_weights():
    """The reference's ONNX export of the v1 checkpoint (yolo_plus.onnx, opset 12), walked node by node with the ONNX
    specification's operator semantics (oracle/onnx_ref.py), against oracle/ncnn_ref.py's reading of the NCNN graph of the
    same checkpoint: identical out0 on the same inputs.  A cross-check of two reference-held graph descriptions (Slice,
    Interp/Resize, Pooling pad mode, Permute and the DFL ordering are read twice, from two formats); it pins no output of
    the reference's engines -- forward parity stays UNPINNED."""
    import torch
    from oracle import ncnn_ref, onnx_ref
    layers = ncnn_ref.load_model(V1_PARAM, V1_BIN)
    nodes, init, g_in, g_out = onnx_ref.read_graph(V1_ONNX)
    assert len(nodes) == 238 and sum(n.op == "Conv" for n in nodes) == 64 and g_in == ["images"] and g_out == ["output0"]
    yy, xx = np.mgrid[0:640, 0:640].astype(np.float32)
    structured = np.stack([0.5 + 0.5 * np.sin(xx / 37.0 + c) * np.cos(yy / 53.0 - c) for c in range(3)])[None]
    inputs = [torch.rand(1, 3, 640, 640, generator=torch.Generator().manual_seed(s)) for s in (0, 1)]
    inputs.append(torch.from_numpy(structured.astype(np.float32)))
    for x in inputs:
        with torch.no_grad():
            a = onnx_ref.run(nodes, init, {"images": x}, g_out)["output0"].numpy()
        b = ncnn_ref.run_graph(layers, x)["out0"].numpy()
        assert a.shape == b.shape == (1, 5, 8400)
        assert np.abs(a[:, 4] - b[:, 4]).max() <= 1e-6                      # scores
        assert np.allclose(a[:, :4], b[:, :4], rtol=1e-6, atol=2e-4)        # boxes in pixels, up to 640: a few fp32 ulps (6e-5 each) between two op orders


def test_synthetic_models_have_the_reference_architecture(synth_models):
    """The exporter reproduces the reference graphs' MAC counts and the oracle
    interpreter runs them."""
    import torch
    from oracle import ncnn_ref
    for preset, macs in (("v1", 1418713600), ("v2", 2542483200)):
        layers = ncnn_ref.load_model(*synth_models[preset])
        assert len(layers) == 206
        assert ncnn_ref.conv_macs(layers) == macs
    out = ncnn_ref.run_graph(layers, torch.rand(1, 3, 640, 640))["out0"]
    assert out.shape == (1, 5, 8400) and torch.isfinite(out).all()


def test_exporter_layer_sequence_equals_reference_graph(synth_models, golden_dir):
    """Layer type, #inputs, #outputs of every line of the reference's v1 NCNN graph (recorded from its model.ncnn.param)."""
    with open(os.path.join(golden_dir, "ref_v1_layer_sequence.json")) as fh:
        ref = json.load(fh)
    mine = [l.split()[:4] for l in open(synth_models["v1"][0]).read().splitlines()[2:]]
    assert len(ref) == len(mine) == 206
    assert all(a == [b[0], int(b[2]), int(b[3])] for a, b in zip(ref, mine))  # layer type, #in, #out


def test_shufflenet_oracle_shapes_and_param_count():
    import torch
    from oracle import shufflenet_ref as S
    sd = S.seeded_state_dict(91)
    n = sum(v.numel() for k, v in sd.items() if "running" not in k and not k.endswith("num_batches_tracked"))
    assert n - 1025 * 91 == 1253604
    m = S.build(91, sd)
    with torch.no_grad():
        y = m(torch.randn(2, 3, 64, 64))
    assert y.shape == (2, 91)


def test_oracle_runs_reference_baseline_graphs(tmp_path):
    """The interpreter covers the op set of the reference's other exported detectors (YOLOv8n, YOLOv5nu with a 6x6 stem,
    YOLO11n with ConvolutionDepthWise / MatMul / Permute / a second Softmax).  The graph files are staged by
    __graft_entry__.build() where /root/reference exists; weights are seeded (none ship with the reference)."""
    import os
    import sys
    import numpy as np
    import pytest
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "yolo-litepi_amd"))
    from litepi import ncnn_export
    from oracle import ncnn_ref
    ran = 0
    for fam in ("yolo8", "yolo5", "yolo11"):
        param = os.path.join(root, "oracle", "_ref", f"{fam}_tt100k.param")
        if not os.path.exists(param):
            continue
        binf = str(tmp_path / f"{fam}.bin")
        ncnn_export.seeded_bin_for_param(param, binf, seed=5)
        layers = ncnn_ref.load_model(param, binf)
        out = ncnn_ref.run_graph(layers, torch.rand(1, 3, 640, 640, generator=torch.Generator().manual_seed(0)))["out0"].numpy()
        assert out.shape == (1, 5, 8400) and np.isfinite(out).all()
        assert (out[0, 4] > 0).all() and (out[0, 4] < 1).all()
        ran += 1
    if ran == 0:
        pytest.skip("reference graph files not staged")


def test_cv2_linear_resize_restatement_properties():
    """oracle.postprocess_ref.resize_linear_u8 (cv2.resize INTER_LINEAR, used by letterbox and by the e2e_optimize ROI stage).
    PARITY UNPINNED (cv2 absent, no fixtures in the reference): pinned by properties and a hand-computed case only."""
    from oracle import postprocess_ref as P
    rng = np.random.default_rng(0)
    const = np.full((37, 23, 3), 91, np.uint8)
    assert (P.resize_linear_u8(const, 64, 64) == 91).all()
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    assert (P.resize_linear_u8(img, 64, 64) == img).all()          # all weights land on one source pixel
    tiny = np.array([[0, 100], [200, 50]], np.uint8)[:, :, None].repeat(3, 2)
    up = P.resize_linear_u8(tiny, 4, 4)[:, :, 0]
    # half-pixel centres: destination columns sample at -0.25, 0.25, 0.75, 1.25 (clamped at the ends); 11-bit coefficients,
    # ((b0*(h0>>4))>>16 + (b1*(h1>>4))>>16 + 2) >> 2 worked by hand for row 1
    assert up[0].tolist() == [0, 25, 75, 100] and up[1].tolist() == [50, 59, 78, 88] and up[3].tolist() == [200, 163, 88, 50], up
    big = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    down = P.resize_linear_u8(big, 64, 64)
    assert down.shape == (64, 64, 3) and abs(float(down.mean()) - float(big.mean())) < 6.0


def test_optimize_roi_rule_differs_from_e2e_where_the_reference_does():
    """oracle.optimize_ref.roi_rects (e2e_optimize.py:480-497) against oracle.postprocess_ref.roi_rects (e2e.py:465-473)."""
    from oracle import optimize_ref as O, postprocess_ref as P
    h, w = 100, 200
    boxes = np.array([[10.9, 20.2, 60.7, 80.9],      # interior: same rectangle under both rules
                      [199.6, 10.0, 200.0, 90.0],    # x1 truncates to 199, x2 = 200: both keep a 1-px column
                      [200.0, 10.0, 200.0, 90.0],    # degenerate at the right edge: e2e.py makes it [199, 200), optimize drops it
                      [-5.5, -3.2, 30.0, 40.0],      # negative corner: truncation toward zero, then clip
                      [50.0, 99.5, 120.0, 100.0]],   # one-row strip at the bottom
                     np.float32)
    r0, v0 = P.roi_rects(boxes, h, w, 50)
    r1, v1 = O.roi_rects(boxes, h, w, 50)
    assert v0 == [0, 1, 2, 3, 4] and v1 == [0, 1, 3, 4]
    assert r1.tolist() == [[10, 20, 60, 80], [199, 10, 200, 90], [0, 0, 30, 40], [50, 99, 120, 100]]
    assert [list(map(int, r)) for r in r0][2] == [199, 10, 200, 90]
    assert O.roi_rects(np.zeros((0, 4), np.float32), h, w)[1] == []
    crops = O.preprocess_rois([np.zeros((5, 7, 3), np.uint8) + 200, np.arange(64 * 64 * 3, dtype=np.uint8).reshape(64, 64, 3)])
    assert crops.shape == (2, 64, 64, 3) and (crops[0] == 200).all() and (crops[1] == np.arange(64 * 64 * 3, dtype=np.uint8).reshape(64, 64, 3)[:, :, ::-1]).all()
    x = O.normalize(crops)
    assert x.shape == (2, 3, 64, 64) and abs(float(x[0].max()) - (200 / 255 - 0.18) / 0.34) < 1e-6


def test_resnet18_oracle_shapes_and_param_count():
    """oracle.resnet_ref: torchvision resnet18 restated (e2e.py:320-323).  11 176 512 backbone parameters + 513 per class
    (torchvision's published count for resnet18 is 11 689 512 at 1000 classes), torchvision's state_dict keys, 64x64 input."""
    import torch
    from oracle import resnet_ref as R
    m = R.build(58, R.seeded_state_dict(58))
    n = sum(p.numel() for p in m.parameters())
    assert n == 11_176_512 + 513 * 58
    assert sum(p.numel() for p in R.ResNet18(1000).parameters()) == 11_689_512
    keys = set(m.state_dict().keys())
    for k in ("conv1.weight", "bn1.running_var", "layer1.0.conv1.weight", "layer2.0.downsample.0.weight", "layer2.0.downsample.1.running_mean",
              "layer4.1.bn2.bias", "fc.weight", "fc.bias"):
        assert k in keys, k
    assert "layer1.0.downsample.0.weight" not in keys
    x = torch.randn(3, 3, 64, 64)
    with torch.no_grad():
        y = m(x)
        f = m.layer4(m.layer3(m.layer2(m.layer1(m.maxpool(m.relu(m.bn1(m.conv1(x))))))))
    assert y.shape == (3, 58) and f.shape == (3, 512, 2, 2) and torch.isfinite(y).all()
    ids, probs = R.predict_batch(m, [np.random.default_rng(0).integers(0, 256, (40, 30, 3), dtype=np.uint8)])
    assert probs.shape == (1, 58) and abs(float(probs.sum()) - 1.0) < 1e-5


def test_mbnet_oracles_have_torchvision_parameter_counts_and_keys():
    """oracle/mbnet_ref.py restates torchvision's mobilenet_v2 / efficientnet_b0 (torchvision is absent here): the parameter
    counts must equal the published ones (3,504,872 / 5,288,548 at 1000 classes) and the state_dict keys torchvision's layout,
    and the backend's random-init fallback must produce exactly those keys and shapes."""
    import torch
    from litepi.backend import random_efficientnet_state, random_mobilenetv2_state
    from oracle import mbnet_ref as M
    for arch, published, rnd, first, last in (("mobilenetv2", 3504872, random_mobilenetv2_state, "features.1.conv.0.0.weight", "features.18.1.running_var"),
                                              ("efficientnet", 5288548, random_efficientnet_state, "features.1.0.block.1.fc1.weight", "features.8.1.running_var")):
        m = M.build(arch, 1000)
        assert sum(p.numel() for p in m.parameters()) == published, arch
        sd = m.state_dict()
        assert first in sd and last in sd and "classifier.1.weight" in sd
        keys = sorted(k for k in sd if not k.endswith("num_batches_tracked"))
        r = rnd(1000)
        assert sorted(r.keys()) == keys
        assert all(tuple(sd[k].shape) == r[k].shape for k in keys)
    x = torch.zeros(1, 3, 64, 64)
    with torch.no_grad():
        assert M.build("mobilenetv2", 58)(x).shape == (1, 58) and M.build("efficientnet", 58)(x).shape == (1, 58)
