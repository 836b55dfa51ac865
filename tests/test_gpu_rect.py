"""Rectangular detector input (lp_config::det_input_h) on the device, and the residual clamp of the 3x3 kernel's
epilogue that it needs.

1. the clamp: a residual 3x3 layer on a map narrower than 20 columns that ConvLayer::build gives the 40-column tile;
2. the two letterbox kernels on (SH, SW), byte-equal to tests/rect_ref.py, geometry bit-equal to lp_letterbox_geometry;
3. out0 in fp32 and fp16 against the oracle at rectangular sizes (and at the square size whose P5 map is 13 columns);
4. lp_detect end to end, the pipeline with BGR / NV12 frames, tracker and inventory, the captured step, the square regression
   and the refusals of the frame-view families.

The oracle forwards are computed once per (model, size, batch) and shared."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pixfmt_ref as PX
import rect_ref as RR

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------- 1. the clamp
@pytest.mark.parametrize("hw", [(7, 13), (13, 13)])
def test_conv3x3_residual_on_a_map_narrower_than_a_strip(hw):
    """3x3, stride 1, 96 -> 96, SiLU, residual, N = 2, fp32: ConvLayer::build gives this shape the 1 x 2 wave tile (40 columns;
    no candidate reaches 60 % use of the map, the two with >= 16-channel chunks that fit the LDS budget are 2x1 and 1x2 waves,
    and the larger chunk, 24 channels, wins), so the second wave's strips start at columns 20..23 of a 13-column map.  Before
    the clamp their residual prefetch read past the row (past the tensor on the last row of the last image); the loads are
    discarded, so the values were right whenever the read did not fault.  Bound: fp32 accumulation over K = 864, as
    test_conv_fp32 (2e-5)."""
    from litepi import Engine
    H, W = hw
    g = torch.Generator().manual_seed(100 * H + W)
    x = torch.randn(2, 96, H, W, generator=g)
    w = torch.randn(96, 96, 3, 3, generator=g) * (1.0 / (96 * 9)) ** 0.5
    b = torch.randn(96, generator=g) * 0.1
    res = torch.randn(2, 96, H, W, generator=g)
    ref = (F.silu(F.conv2d(x.double(), w.double(), b.double(), padding=1)) + res.double()).numpy()
    e = Engine(precision="fp32", max_batch=2)
    try:
        y = e.test_conv(x.numpy(), w.numpy(), b.numpy(), stride=1, act=1, res=res.numpy())
    finally:
        e.close()
    err = np.abs(y - ref).max()
    print(f"conv3x3 96->96 res silu fp32 on {H}x{W}: max err {err:.3e}")
    assert err < 2e-5, f"max abs err {err}"


# ---------------------------------------------------------------------------- 2. letterbox
LB_CASES = [((384, 640), (1080, 1920)), ((384, 640), (720, 1280)), ((384, 640), (480, 640)), ((384, 640), (37, 100)),
            ((384, 640), (384, 640)), ((640, 384), (640, 360)), ((640, 384), (1920, 1080)), ((224, 416), (1080, 1920)),
            ((224, 416), (100, 4480)), ((384, 640), (50, 2600))]


@pytest.fixture(scope="module")
def lb_engines():
    from litepi import Engine
    engs = {}

    def get(shape):
        if shape not in engs:
            engs[shape] = Engine(precision="fp16", max_batch=1, det_input=shape)
        return engs[shape]
    yield get
    for e in engs.values():
        e.close()


def tiled_rows_fit(det_w_new, w):
    """launch_letterbox's rule (misc_kernels.hip): the LDS row of a 128-column tile, 16 rows of it within 64 KiB"""
    span = int((128.0 * (w / max(det_w_new, 1)) + 4.0) * 3.0) + 32
    return ((span + 15) & ~15) * 16 <= 64 * 1024


@pytest.mark.parametrize("shape,hw", LB_CASES, ids=[f"{h}x{w}_into_{s[0]}x{s[1]}" for s, (h, w) in LB_CASES])
def test_letterbox_kernels_equal_rect_ref(lb_engines, shape, hw):
    """Both kernels (the launcher's choice = the tiled one where its LDS rows fit, and the per-pixel one) byte-equal to
    rect_ref.letterbox; ratio and pads bit-equal to lp_letterbox_geometry.  100 x 4480 into 224 x 416 is a 10.8 x down-scale:
    a tile row spans 4179 source bytes, 16 rows of 4192 are 67072 > 65536 bytes, so the launcher itself takes the per-pixel
    kernel there.  50 x 2600 into 384 x 640 is a 4.06 x down-scale over five column tiles: staged, with the span's first byte
    far beyond the LDS shift from the second tile on."""
    from litepi.backend import letterbox_geometry
    SH, SW = shape
    rng = np.random.default_rng(hw[0] * 7 + hw[1] + SH)
    img = rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
    exp, _, _ = RR.letterbox(img, SH, SW)
    geo = letterbox_geometry(SH, SW, hw[0], hw[1])
    ref_geo = RR.letterbox_geometry(SH, SW, hw[0], hw[1])
    assert tiled_rows_fit(ref_geo["new_w"], hw[1]) == (hw != (100, 4480))
    e = lb_engines(shape)
    for per_pixel in (False, True):
        got, r, (pw, ph) = e.test_letterbox(img, per_pixel=per_pixel)
        assert got.shape == exp.shape == (SH, SW, 3)
        for name, v in (("ratio", r), ("pad_w", pw), ("pad_h", ph)):
            assert np.float32(v).tobytes() == np.float32(geo[name]).tobytes() == np.float32(ref_geo[name]).tobytes(), name
        assert np.array_equal(got, exp), f"per_pixel={per_pixel}: max diff {np.abs(got.astype(int) - exp.astype(int)).max()}"


# ---------------------------------------------------------------------------- 3. out0
@pytest.fixture(scope="module")
def rect_models(tmp_path_factory):
    """seeded v1 / v2 detectors exported at a size (one seed = one set of weights at every size), and their oracle out0 on
    seeded images, computed once per (preset, size, batch)"""
    from litepi import ncnn_export
    from oracle import ncnn_ref
    d = tmp_path_factory.mktemp("rect_models")
    files, refs = {}, {}

    def model(preset, size):
        if (preset, size) not in files:
            p, b = str(d / f"{preset}_{size[0]}x{size[1]}.param"), str(d / f"{preset}_{size[0]}x{size[1]}.bin")
            ncnn_export.export_detector(p, b, preset, seed=77, cls_bias=-2.0, size=size if size[0] != size[1] else size[0])
            files[(preset, size)] = (p, b)
        return files[(preset, size)]

    def ref(preset, size, batch):
        if (preset, size, batch) not in refs:
            p, b = model(preset, size)
            imgs = np.random.default_rng(5 + batch).integers(0, 256, (batch, size[0], size[1], 3), dtype=np.uint8)
            out = RR.out0(ncnn_ref.load_model(p, b), imgs)
            imgs.setflags(write=False)
            out.setflags(write=False)
            refs[(preset, size, batch)] = (imgs, out)
        return refs[(preset, size, batch)]
    return model, ref


FP32_CASES = [(pr, s, b, c) for s, b, c in (((384, 640), 3, 3), ((640, 384), 2, 2), ((320, 640), 5, 5), ((224, 416), 2, 2), ((384, 640), 3, 64))
              for pr in ("v1", "v2")] + [("v2", (416, 416), 2, 2)]


@pytest.mark.parametrize("preset,size,batch,cap", FP32_CASES, ids=[f"{p}_{s[0]}x{s[1]}x{b}cap{c}" for p, s, b, c in FP32_CASES])
def test_out0_fp32_rectangular(rect_models, preset, size, batch, cap):
    """fp32 out0 against the oracle at the documented bound (score 1e-3, box abs + rel 1e-3, as
    test_detector_fp32_plans_and_sizes).  320 x 640: the P5 map is 10 x 20, no whole-image 20 x 20 kernel applies.  v2 at
    224 x 416 x 2 is the case that faulted before the epilogue's clamp; v2 at the square 416 x 2 read past the residual tensor
    in the same launches.  384 x 640 also on a handle of capacity 64 (other tile shapes and channel splits)."""
    from litepi import Engine
    model, ref = rect_models
    p, b = model(preset, size)
    imgs, want = ref(preset, size, batch)
    e = Engine(precision="fp32", max_batch=cap, det_input=size)
    try:
        e.load_detector(p, b)
        assert e.num_anchors == sum((size[0] // s) * (size[1] // s) for s in (8, 16, 32))
        got = e.detect_raw(imgs)
    finally:
        e.close()
    assert got.shape == want.shape == (batch, 5, e.num_anchors)
    err_box = np.abs(got[:, :4] - want[:, :4])
    err_s = np.abs(got[:, 4] - want[:, 4]).max()
    print(f"fp32 {preset} {size[0]}x{size[1]} x{batch} cap {cap}: score err {err_s:.3e}, box err {err_box.max():.3e} px")
    assert (err_box <= 1e-3 + 1e-3 * np.abs(want[:, :4])).all(), f"box rows: max err {err_box.max()}"
    assert err_s <= 1e-3, f"score row: max err {err_s}"


@pytest.mark.parametrize("preset", ["v1", "v2"])
@pytest.mark.parametrize("size", [(384, 640), (224, 416)], ids=["384x640", "224x416"])
def test_out0_fp16_rectangular_both_plans(rect_models, monkeypatch, preset, size):
    """fp16 out0 on both plans (LITEPI_NO_C2F=1 = the layer plan, as test_detector_fp16_c2f_plan_other_sizes selects them; a
    handle of 4 images, the capacity from which the whole-C2f launches are planned) at that test's documented bounds: score
    0.02 (v2: 0.025), box 0.35 cells of the anchor's level, mean box error 0.5 px; the stride per anchor from
    rect_ref.anchor_table.  The layer plan must hold no whole-C2f / s2conv launch."""
    from litepi import Engine
    model, ref = rect_models
    batch = 4
    p, b = model(preset, size)
    imgs, want = ref(preset, size, batch)
    _, stride = RR.anchor_table(*size)
    got, names = {}, {}
    for plan in ("layer", "c2f"):
        if plan == "layer":
            monkeypatch.setenv("LITEPI_NO_C2F", "1")
        else:
            monkeypatch.delenv("LITEPI_NO_C2F", raising=False)
        e = Engine(precision="fp16", max_batch=batch, det_input=size)
        try:
            e.load_detector(p, b)
            got[plan] = e.detect_raw(imgs)
            e.profile_next(True)
            e.detect_raw(imgs)
            names[plan] = [k["name"] for k in e.profile_read()]
        finally:
            e.close()
    fused = sorted({n for n in names["c2f"] if n.startswith("c2f<") or n.startswith("s2conv")})
    print(f"fp16 {preset} {size[0]}x{size[1]} x{batch}: {len(names['c2f'])} launches ({len(names['layer'])} in the layer plan), fused: {fused}")
    assert not any(n.startswith("c2f<") or n.startswith("s2conv<") for n in names["layer"])
    assert not any(n.startswith("sppf<") for n in names["c2f"]), "the whole-image SPPF kernel is for 20 x 20 maps only"
    doc_score = 0.02 if preset == "v1" else 0.025
    for plan in ("layer", "c2f"):
        g = got[plan]
        es, eb = np.abs(g[:, 4] - want[:, 4]), np.abs(g[:, :4] - want[:, :4])
        cells = (eb / stride).max()
        print(f"   {plan:5s} plan: score err max {es.max():.4f}; box err max {eb.max():.3f} px = {cells:.3f} cells, mean {eb.mean():.4f}")
        assert es.max() <= doc_score, f"{plan}: score error {es.max()}"
        assert cells <= 0.35, f"{plan}: box error {cells} cells"
        assert eb.mean() <= 0.5, f"{plan}: mean box error {eb.mean()}"
    if names["c2f"] == names["layer"]:
        assert np.array_equal(got["c2f"], got["layer"])


# ---------------------------------------------------------------------------- 4. end to end
def pick_conf(scores, lo=3, hi=32, gap=2.2e-3):
    """the lowest threshold among a frame's lo-th .. hi-th highest scores that sits in the middle of a gap wider than `gap`
    (more than twice the fp32 score bound of 1e-3), and its distance to the two neighbours: no candidate is borderline, so the
    comparison leaves nothing out.  (0.0, 0.0) when the frame has no such gap."""
    s = np.sort(np.asarray(scores, np.float64).ravel())[::-1][:hi + 1]
    for k in range(hi - 1, lo - 1, -1):
        if s[k] - s[k + 1] > gap:
            return float(0.5 * (s[k] + s[k + 1])), float(0.5 * (s[k] - s[k + 1]))
    return 0.0, 0.0


def scene(seed, H, W, n=12):
    """noise with n flat rectangles: the seeded random detector scores pure noise almost uniformly"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    for _ in range(n):
        h, w = rng.integers(24, 120, 2)
        y, x = rng.integers(0, H - h), rng.integers(0, W - w)
        f[y:y + h, x:x + w] = rng.integers(0, 256, 3)
    return f


@pytest.fixture(scope="module")
def e2e_case(rect_models):
    """two frames (1080 x 1920, 480 x 640), the v1 model at 384 x 640 and, on the CPU, the threshold and the oracle's detections"""
    from oracle import ncnn_ref
    model, _ = rect_models
    p, b = model("v1", (384, 640))
    layers = ncnn_ref.load_model(p, b)
    frames = [np.random.default_rng(99).integers(0, 256, (1080, 1920, 3), dtype=np.uint8), scene(101, 480, 640)]
    lbs = np.stack([RR.letterbox(f, 384, 640)[0] for f in frames])
    scores = RR.out0(layers, lbs)[:, 4]
    confs = []
    for s in scores:   # a threshold per frame: the frames go through lp_detect one by one
        conf, margin = pick_conf(s)
        assert margin > 1e-3, f"no score gap of twice the fp32 score bound (1e-3) around a threshold (margin {margin})"
        confs.append(conf)
    want = [RR.detect(layers, f, 384, 640, c, 0.45) for f, c in zip(frames, confs)]
    return p, b, frames, confs[0], want, confs


def test_lp_detect_equals_rect_ref(e2e_case):
    """lp_detect in fp32 on a 384 x 640 handle against rect_ref.detect (letterbox -> oracle forward -> postprocess), a frame
    per call.  Each frame's threshold sits more than 1e-3 (the fp32 score bound) from both neighbouring scores among its 4th
    to 32nd highest (chosen and checked on the CPU from the oracle alone), so no candidate is borderline and nothing is left
    out of the comparison: the same number of boxes per frame, every box within 0.05 px and every score within 1e-3 of its
    match, classes equal (test_detect_non_square_images_fp32's bounds), boxes inside the frame."""
    from litepi import NCNNDetector
    p, b, frames, _, want, confs = e2e_case
    det = NCNNDetector(p, b, (384, 640), precision="fp32", max_batch=2, max_det=300)
    try:
        got = [det.detect(f, c, 0.45) for f, c in zip(frames, confs)]
    finally:
        det.engine.close()
    total = 0
    for f, conf, (gb, gs, gc), (eb, es, ec) in zip(frames, confs, got, want):
        print(f"lp_detect 384x640 on {f.shape[0]}x{f.shape[1]}: {len(gb)} boxes, oracle {len(eb)} (conf {conf:.4f})")
        assert len(gb) == len(eb)
        for box, sc, cl in zip(eb, es, ec):
            d = np.abs(gb - box).max(axis=1)
            j = int(np.argmin(d))
            assert d[j] <= 0.05 and abs(gs[j] - sc) <= 1e-3 and gc[j] == cl, (box, gb[j])
        if len(gb):
            assert gb[:, [0, 2]].max() <= f.shape[1] and gb[:, [1, 3]].max() <= f.shape[0] and gb.min() >= 0
        total += len(gb)
    assert total >= 8, "too few detections for a meaningful test"


@pytest.fixture(scope="module")
def pipe_models(tmp_path_factory, e2e_case):
    from litepi.backend import random_shufflenet_state
    d = tmp_path_factory.mktemp("rect_pipe")
    sd = random_shufflenet_state(91, seed=3)
    cls_file = str(d / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, cls_file)
    return sd, cls_file


N_CALLS, N_FRAMES = 3, 2
TCFG = dict(n_streams=N_FRAMES, max_tracks=256, max_age=0, min_hits=1, iou_match=0.5)


def clip(rng, H, W):
    base = rng.integers(0, 256, (N_FRAMES, H, W, 3), dtype=np.uint8)
    patch = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    calls = []
    for k in range(N_CALLS):
        f = base.copy()
        f[:, 200:296, 160 + 4 * k:256 + 4 * k] = patch
        calls.append(f)
    return calls


def clip_conf(p, b, frames_bgr, size=(384, 640)):
    """a threshold that at least three anchors of every given frame pass with a margin of 0.1 in the logit, from the device's
    own fp16 scores (as the model fixtures of tests/test_gpu_inventory.py and tests/test_gpu_tracking.py calibrate): it only
    makes the frames produce records, no bound depends on it"""
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=len(frames_bgr), det_input=size)
    try:
        e.load_detector(p, b)
        lb = np.stack([e.test_letterbox(f)[0] for f in frames_bgr])
        s = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64), axis=1)[:, ::-1]
    finally:
        e.close()
    third = s[:, 2].min()
    return float(1 / (1 + np.exp(-(np.log(third / (1 - third)) - 0.1))))


@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_pipeline_host_frames_equal_device_frames(e2e_case, pipe_models, fmt):
    """HybridPipeline.run_batch(track, inventory) at 384 x 640 over three calls of two 720 x 1280 frames (BGR, NV12) against
    the device-frame path on a second handle (lp_run_batch_device -> lp_track_device -> lp_inventory_device): the records,
    the tracks and the drained signs with their crops are byte-equal, and something was detected and logged."""
    from litepi import Engine, HybridPipeline
    from litepi._ffi import DET_DTYPE, TRACK_DTYPE
    p, b = e2e_case[:2]
    sd, cls_file = pipe_models
    H, W, B = 720, 1280, N_FRAMES
    calls = clip(np.random.default_rng(31), H, W)
    if fmt == "nv12":
        calls = [np.stack([PX.bgr_to_nv12(f) for f in c]) for c in calls]
        conf = clip_conf(p, b, [PX.nv12_to_bgr(f, "bt601") for c in calls for f in c])
    else:
        conf = clip_conf(p, b, [f for c in calls for f in c])
    sid = np.arange(B, dtype=np.int32)
    pipe = HybridPipeline(p, b, cls_file, "shufflenetv2", num_classes=91, det_input_size=(384, 640), precision="fp16", max_batch=B,
                          max_det=300, pixel_format=fmt, track=True, track_config=TCFG, inventory=dict(best="area"))
    host = []
    try:
        for frames in calls:
            host.append(pipe.run_batch(list(frames), conf, 0.45, 50, stream_ids=sid))
        pipe.engine.inventory_flush(-1)
        hs, hc, hd = pipe.engine.inventory_drain(crops=True)
    finally:
        pipe.close()
    dev = torch.device("cuda", 0)
    eng = Engine(precision="fp16", max_batch=B, max_det=300, num_classes=91, det_input=(384, 640))
    try:
        eng.load_detector(p, b)
        eng.load_classifier(sd)
        eng.set_input_format(fmt, "bt601")
        eng.tracker_create(**TCFG)
        eng.inventory_create(best="area")
        d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        t = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        total = 0
        for k, frames in enumerate(calls):
            x = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
            eng.run_batch_device(x.data_ptr(), B, H, W, conf, 0.45, 50, d.data_ptr(), c.data_ptr())
            eng.track_device(d.data_ptr(), c.data_ptr(), B, t.data_ptr(), sid)
            eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), B, sid, crops=True)
            torch.cuda.synchronize()
            eng.debug_rois()   # synchronises the engine's stream
            counts = c.cpu().numpy()[:B]
            dets = d.cpu().numpy().view(DET_DTYPE).reshape(B, 300)
            tracks = t.cpu().numpy().view(TRACK_DTYPE).reshape(B, 300)
            for i in range(B):
                res, met = host[k][i]
                n = int(counts[i])
                assert len(res) == n, f"{fmt} call {k} frame {i}: {len(res)} host results, {n} device records"
                dd, tt = dets[i, :n], tracks[i, :n]
                assert [r["bbox"] for r in res] == list(map(tuple, np.stack([dd["x1"], dd["y1"], dd["x2"], dd["y2"]], 1).astype(int).tolist()))
                assert np.array_equal(np.array([r["det_conf"] for r in res], np.float32), dd["det_conf"])
                assert np.array_equal(np.array([r["cls_conf"] for r in res], np.float32), dd["cls_conf"])
                assert [r["cls_class"] for r in res] == dd["cls_class"].tolist()
                assert [r["track_id"] for r in res] == tt["track_id"].tolist()
                assert [r["track_hits"] for r in res] == tt["hits"].tolist()
                total += n
        eng.inventory_flush(-1)
        ds, dc, ddrop = eng.inventory_drain(crops=True)
    finally:
        eng.close()
    print(f"{fmt}: {total} records over {N_CALLS} calls, {len(ds)} signs")
    assert total >= 6 and len(ds) >= 1
    ho, do = np.argsort(hs["stream"], kind="stable"), np.argsort(ds["stream"], kind="stable")
    assert hs[ho].tobytes() == ds[do].tobytes() and hd == ddrop
    assert hc[ho].tobytes() == dc[do].tobytes()


def test_captured_step_replays_on_a_rectangular_handle(e2e_case, pipe_models):
    """lp_run_batch_device on a 384 x 640 handle: the first call runs eagerly, the second is captured, the third and fourth
    replay the graph; every call returns the same counts and records, and a batch of another shape in between does not disturb them"""
    from litepi import Engine
    p, b, frames = e2e_case[:3]
    sd, _ = pipe_models
    dev = torch.device("cuda", 0)
    B, H, W = 2, 480, 640
    imgs = np.stack([frames[1], frames[1][::-1].copy()])
    conf = clip_conf(p, b, list(imgs) + [frames[0]])
    eng = Engine(precision="fp16", max_batch=B, max_det=300, num_classes=91, det_input=(384, 640))
    try:
        eng.load_detector(p, b)
        eng.load_classifier(sd)
        x = torch.from_numpy(imgs).to(dev)
        x1 = torch.from_numpy(np.ascontiguousarray(frames[0][None])).to(dev)
        d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
        outs = []
        for k in range(4):
            if k == 3:
                eng.run_batch_device(x1.data_ptr(), 1, 1080, 1920, conf, 0.45, 50, d.data_ptr(), c.data_ptr())
            d.zero_(); c.zero_()
            torch.cuda.synchronize()
            eng.run_batch_device(x.data_ptr(), B, H, W, conf, 0.45, 50, d.data_ptr(), c.data_ptr())
            eng.synchronize()
            cnt = c.cpu().numpy()
            recs = d.cpu().numpy().reshape(B, 300 * 32)
            # the three count words per frame and each frame's kept records (what lies behind them is unspecified)
            outs.append((cnt.tobytes(), [recs[i, :32 * int(cnt[i])].tobytes() for i in range(B)]))
        n = np.frombuffer(outs[0][0], np.int32)[:B]
    finally:
        eng.close()
    assert n.sum() >= 2, "nothing detected"
    for k, o in enumerate(outs[1:], 1):
        assert o == outs[0], f"call {k} differs from the eager call"


def test_det_input_h_equal_to_det_input_is_the_square_handle(synth_models):
    """lp_config::det_input_h = 640 on a 640 handle (Engine(det_input=(640, 640))): out0 and lp_detect's records byte-equal to
    det_input_h = 0 (Engine(det_input=640)); the frame views stay available"""
    from litepi import Engine
    p, b = synth_models["v1"]
    rng = np.random.default_rng(8)
    imgs = rng.integers(0, 256, (2, 640, 640, 3), dtype=np.uint8)
    frames = [rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8), rng.integers(0, 256, (600, 500, 3), dtype=np.uint8)]
    got, conf = [], clip_conf(p, b, frames, size=640)
    for size in (640, (640, 640)):
        e = Engine(precision="fp16", max_batch=2, det_input=size)
        try:
            assert e.cfg.det_input_h == (0 if size == 640 else 640) and e.cfg.det_input == 640
            e.load_detector(p, b)
            out0 = e.detect_raw(imgs)
            dets, counts = e.detect(frames, conf, 0.45)
            views = e.test_view_windows(frames[0], ["full"])
            got.append((out0.tobytes(), dets.tobytes(), counts.tolist(), views.tobytes()))
        finally:
            e.close()
    assert got[0][3] == got[1][3], "the whole-frame view differs"
    assert got[0][0] == got[1][0], "out0 differs"
    assert got[0][2] == got[1][2] and got[0][1] == got[1][1], "records differ"
    assert sum(got[0][2]) >= 1


def test_frame_views_refuse_a_rectangular_handle(e2e_case, pipe_models):
    """every tiled, views and focus entry point on a 384 x 640 handle: LP_ERR_STATE with a message that names the shape, before
    anything is enqueued; the handle then still runs lp_run_batch and gives the result it gave before"""
    from litepi import Engine
    from litepi._ffi import LP_ERR_STATE, LitepiError
    p, b, frames = e2e_case[:3]
    sd, _ = pipe_models
    dev = torch.device("cuda", 0)
    f = frames[1]
    conf = clip_conf(p, b, [f])
    H, W = f.shape[:2]
    eng = Engine(precision="fp16", max_batch=8, max_det=300, num_classes=91, det_input=(384, 640))
    try:
        eng.load_detector(p, b)
        eng.load_classifier(sd)
        eng.tracker_create(n_streams=1)
        before = eng.run_batch([f], conf, 0.45, 50)
        x = torch.from_numpy(f[None].copy()).to(dev)
        d = torch.zeros(8 * 300 * 32, dtype=torch.uint8, device=dev)
        c = torch.zeros(3 * 8, dtype=torch.int32, device=dev)
        args = (x.data_ptr(), 1, H, W, conf, 0.45, 50, d.data_ptr(), c.data_ptr())
        calls = {
            "lp_run_tiled": lambda: eng.run_tiled([f], conf, 0.45, 50, overlap=64),
            "lp_run_tiled_device": lambda: eng.run_tiled_device(*args, overlap=64),
            "lp_run_views": lambda: eng.run_views([f], ["full", (0, 0, 320, 240)], conf, 0.45, 50),
            "lp_run_views_device": lambda: eng.run_views_device(x.data_ptr(), 1, H, W, ["full"], conf, 0.45, 50, d.data_ptr(), c.data_ptr()),
            "lp_focus_create": lambda: eng.focus_create(slots=2),
            "lp_focus_plan": lambda: eng.focus_plan([H], [W]),
            "lp_run_focus": lambda: eng.run_focus([f], conf, 0.45, 50),
            "lp_run_focus_device": lambda: eng.run_focus_device(*args),
            "lp_test_tile_views": lambda: eng.test_tile_views(f, overlap=64),
            "lp_test_view_windows": lambda: eng.test_view_windows(f, ["full"]),
        }
        for name, call in calls.items():
            with pytest.raises(LitepiError) as ei:
                call()
            assert ei.value.code == LP_ERR_STATE, f"{name}: code {ei.value.code}: {ei.value}"
            assert "384x640" in str(ei.value) and name in str(ei.value), f"{name}: {ei.value}"
        after = eng.run_batch([f], conf, 0.45, 50)
    finally:
        eng.close()
    assert before[1].tolist() == after[1].tolist() and before[0].tobytes() == after[0].tobytes()
    assert int(before[1][0]) >= 1
