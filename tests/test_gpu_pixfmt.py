"""GPU tests of the NV12 front door (include/litepi.h lp_frame_format), everything through the C-ABI.

1. the converter alone (lp_test_convert_frames) is bit-exact against the int64 oracle of tests/pixfmt_ref.py;
2. every frame-taking entry point gives on NV12 frames byte-for-byte what it gives on the BGR frames the oracle makes from them;
3. the format is handle state: BGR -> NV12 -> BGR on one handle, and two NV12 layouts alternating over the SAME buffers, never
   replay a step captured for another layout;
4. every layout error is LP_ERR_ARG at the call that sees it, and the handle stays usable;
5. the Python surface (HybridPipeline, e2e --raw_frames) returns what it returns for the converted frames.
"""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import pixfmt_ref as R

pytestmark = pytest.mark.gpu

CONF, IOU, MIN_AREA = 0.25, 0.45, 50


# ---------------------------------------------------------------------------- 1. the converter
@pytest.fixture(scope="module")
def conv_eng():
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=64, max_det=8, num_classes=4)
    yield e
    e.close()


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_converter_all_2_24_inputs(conv_eng, matrix):
    frames = R.all_yuv_frames()
    got = conv_eng.test_convert_frames(np.stack(frames), 64, 512, 512, matrix=matrix)
    for i, f in enumerate(frames):
        want = R.nv12_to_bgr(f, matrix)
        assert np.array_equal(got[i], want), f"{matrix}: frame {i} differs in {int((got[i] != want).sum())} bytes"


@pytest.mark.parametrize("H,W", [(2, 2), (2, 16), (6, 18), (640, 640), (682, 1198), (2048, 2048)], ids=lambda v: str(v))
@pytest.mark.parametrize("B", [1, 3])
def test_converter_sizes_and_byte_offsets(conv_eng, H, W, B):
    rng = np.random.default_rng(H * 7 + W + B)
    frames = [rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8) for _ in range(B)]
    want = np.stack([R.nv12_to_bgr(f, "bt601") for f in frames])
    for off in (0, 1, 3, 8, 16, 63):
        got = conv_eng.test_convert_frames(np.stack(frames), B, H, W, byte_offset=off)   # (the hook itself checks its guard bytes)
        assert np.array_equal(got, want), f"{W}x{H} B={B} byte_offset={off}: {int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("pitch", [1922, 1936, 2048])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_converter_pitched_frames_with_plane_gap(conv_eng, pitch, matrix):
    H, W, B = 270, 1920, 2
    rng = np.random.default_rng(pitch)
    frames = [rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8) for _ in range(B)]
    want = np.stack([R.nv12_to_bgr(f, matrix) for f in frames])
    for gap, tail, off in ((3 * pitch + 6, 100, 0), (16 * pitch, 0, 0), (2 * pitch + 1, 37, 5)):
        buf, uv, fb, st = R.pack_frames(frames, pitch=pitch, uv_offset=pitch * H + gap, frame_stride=pitch * H + gap + pitch * (H // 2) + tail)
        got = conv_eng.test_convert_frames(buf, B, H, W, matrix=matrix, pitch=pitch, uv_offset=uv, frame_stride=st, byte_offset=off)
        assert np.array_equal(got, want), f"pitch {pitch} gap {gap} stride tail {tail} offset {off}: {int((got != want).sum())} bytes differ"


# ---------------------------------------------------------------------------- models and frames of the pipeline tests
def _noise_nv12(rng, H, W):
    """an NV12 frame made with the forward helper from the BGR noise the device-path tests use, and its BGR conversion"""
    nv = R.bgr_to_nv12(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    return nv, R.nv12_to_bgr(nv, "bt601")


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(2024)
    sets = {"640": [_noise_nv12(rng, 640, 640) for _ in range(3)],          # the no-letterbox path
            "720p": [_noise_nv12(rng, 720, 1280) for _ in range(2)]}
    sets["mixed"] = [sets["640"][0], sets["720p"][1], _noise_nv12(rng, 482, 366)]   # (366 is not a multiple of 16)
    return sets


@pytest.fixture(scope="module")
def models(tmp_path_factory, frames):
    """seeded v1 / v2 detectors whose class bias is shifted so that on EVERY frame of the test sets at least three anchors pass
    conf 0.25 with a margin of 0.1 in the logit (fp16 and fp32 then agree that something is found), measured with the
    device's own scores on the letterboxed BGR frames"""
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    d = tmp_path_factory.mktemp("pixfmt_models")
    out = {"cls": random_shufflenet_state(91, seed=3)}
    every = [bgr for s in ("640", "720p", "mixed") for _, bgr in frames[s]]
    for preset in ("v1", "v2"):
        p, b = str(d / f"{preset}.param"), str(d / f"{preset}.bin")
        ncnn_export.export_detector(p, b, preset, seed=4321, cls_bias=0.0)
        e = Engine(precision="fp16", max_batch=len(every), max_det=300, num_classes=91)
        try:
            e.load_detector(p, b)
            lb = np.stack([e.test_letterbox(f)[0] for f in every])
            s = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64), axis=1)[:, ::-1]
        finally:
            e.close()
        third = s[:, 2].min()
        ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - (np.log(third / (1 - third)) - 0.1)))
        out[preset] = (p, b)
    return out


def _engine(models, preset, prec, max_batch=16, classifier=True):
    from litepi import Engine
    e = Engine(precision=prec, max_batch=max_batch, max_det=300, num_classes=91)
    e.load_detector(*models[preset])
    if classifier:
        e.load_classifier(models["cls"])
    return e


def _set_fmt(eng, **kw):
    """lp_set_input_format with raw field values (no Python-side validation); returns the status"""
    from litepi._ffi import LpFrameFormat
    f = LpFrameFormat()
    for k, v in kw.items():
        if k == "reserved":
            f.reserved[v] = 1
        else:
            setattr(f, k, v)
    return eng.lib.lp_set_input_format(eng._h, C.byref(f))


def _host_call(eng, entry, bufs, sizes, tiling=None):
    """lp_detect / lp_run_batch / lp_run_tiled on raw frame buffers (1-D or n-D uint8 arrays, any layout) -> (status, result)
    with result = (records per frame as bytes, counts, pre-filter counts, mean-score bits)"""
    from litepi._ffi import DET_DTYPE, LpTiling, LpTiming
    B = len(bufs)
    keep = [np.ascontiguousarray(b, dtype=np.uint8) for b in bufs]
    ptrs = (C.c_void_p * B)(*[k.ctypes.data for k in keep])
    hs = (C.c_int * B)(*[s[0] for s in sizes])
    ws = (C.c_int * B)(*[s[1] for s in sizes])
    dets = np.zeros((B, eng.cfg.max_det), dtype=DET_DTYPE)
    counts, num_det, avg, timing = (C.c_int * B)(), (C.c_int * B)(), (C.c_float * B)(), LpTiming()
    if entry == "detect":
        rc = eng.lib.lp_detect(eng._h, ptrs, hs, ws, B, CONF, IOU, dets.ctypes.data, counts)
    elif entry == "run_batch":
        rc = eng.lib.lp_run_batch(eng._h, ptrs, hs, ws, B, CONF, IOU, MIN_AREA, dets.ctypes.data, counts, num_det, avg, C.byref(timing))
    else:
        t = LpTiling()
        t.overlap, t.full_frame = tiling or (128, 1)
        rc = eng.lib.lp_run_tiled(eng._h, ptrs, hs, ws, B, C.byref(t), CONF, IOU, MIN_AREA, dets.ctypes.data, counts, num_det, avg,
                                  C.byref(timing))
    cnt = np.array(counts[:], dtype=np.int64)
    recs = [dets[i, :cnt[i]].tobytes() for i in range(B)] if rc == 0 else []
    return rc, (recs, cnt, np.array(num_det[:], dtype=np.int64), np.array(avg[:], dtype=np.float32).view(np.uint32), dets, timing)


def _device_call(eng, entry, dev_buf, B, H, W, res):
    """lp_run_batch_device / lp_run_tiled_device -> (status, result) in the shape of _host_call"""
    from litepi._ffi import DET_DTYPE, LpTiling
    dd, dc = res
    if entry == "run_batch_device":
        rc = eng.lib.lp_run_batch_device(eng._h, C.c_void_p(dev_buf.data_ptr()), B, H, W, CONF, IOU, MIN_AREA, C.c_void_p(dd.data_ptr()),
                                         C.c_void_p(dc.data_ptr()))
    else:
        t = LpTiling()
        t.overlap, t.full_frame = 128, 1
        rc = eng.lib.lp_run_tiled_device(eng._h, C.c_void_p(dev_buf.data_ptr()), B, H, W, C.byref(t), CONF, IOU, MIN_AREA,
                                         C.c_void_p(dd.data_ptr()), C.c_void_p(dc.data_ptr()))
    if rc != 0:
        return rc, None
    eng.synchronize()
    torch.cuda.synchronize()
    cnt = dc.cpu().numpy()
    dets = dd.cpu().numpy().view(DET_DTYPE).reshape(-1, eng.cfg.max_det)
    kept = cnt[:B].astype(np.int64)
    return rc, ([dets[i, :kept[i]].tobytes() for i in range(B)], kept, cnt[B:2 * B].astype(np.int64), cnt[2 * B:3 * B].view(np.uint32).copy(),
                dets.copy(), None)


def _result_buffers(eng, B):
    return (torch.zeros(B * eng.cfg.max_det * 32, dtype=torch.uint8, device="cuda"), torch.zeros(3 * B, dtype=torch.int32, device="cuda"))


def _same(a, b, tag, classified=True):
    assert np.array_equal(a[1], b[1]), f"{tag}: kept counts differ ({a[1]} vs {b[1]})"
    assert a[0] == b[0], f"{tag}: records differ"
    if classified:
        assert np.array_equal(a[2], b[2]), f"{tag}: pre-filter counts differ"
        assert np.array_equal(a[3], b[3]), f"{tag}: mean score bits differ"


def _not_vacuous(r, tag, classified=True):
    assert int(r[1].sum()) >= 1, f"{tag}: no kept box, the comparison is empty"
    if classified:
        n_cls = sum(int((r[4][i, :r[1][i]]["cls_class"] >= 0).sum()) for i in range(len(r[1])))
        assert n_cls >= 1, f"{tag}: no classified ROI, the comparison is empty"


# ---------------------------------------------------------------------------- 2. pipeline identity
@pytest.mark.parametrize("preset", ["v1", "v2"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_pipeline_identity_nv12_vs_converted_bgr(models, frames, preset, prec):
    eng = _engine(models, preset, prec)
    n_checked = 0
    try:
        for set_name, fs in frames.items():
            nv = [f[0] for f in fs]
            bgr = [f[1] for f in fs]
            sizes = [b.shape[:2] for b in bgr]
            B = len(fs)
            for entry in ("detect", "run_batch", "run_tiled"):
                tag = f"{preset} {prec} {set_name} {entry}"
                assert _set_fmt(eng) == 0
                rc, ref = _host_call(eng, entry, bgr, sizes)
                assert rc == 0, f"{tag} BGR: {eng.lib.lp_last_error()}"
                assert _set_fmt(eng, pixfmt=1) == 0
                rc, got = _host_call(eng, entry, nv, sizes)
                assert rc == 0, f"{tag} NV12: {eng.lib.lp_last_error()}"
                _same(got, ref, tag, classified=entry != "detect")
                _not_vacuous(ref, tag, classified=entry != "detect")
                n_checked += int(ref[1].sum())
            if set_name == "mixed":
                continue   # the device entry points take frames of one size
            H, W = sizes[0]
            d_bgr, d_nv = torch.from_numpy(np.stack(bgr)).cuda(), torch.from_numpy(np.stack(nv)).cuda()
            res = _result_buffers(eng, B)
            for entry in ("run_batch_device", "run_tiled_device"):
                tag = f"{preset} {prec} {set_name} {entry}"
                assert _set_fmt(eng) == 0
                rc, ref = _device_call(eng, entry, d_bgr, B, H, W, res)
                assert rc == 0, f"{tag} BGR: {eng.lib.lp_last_error()}"
                assert _set_fmt(eng, pixfmt=1) == 0
                rc, got = _device_call(eng, entry, d_nv, B, H, W, res)
                assert rc == 0, f"{tag} NV12: {eng.lib.lp_last_error()}"
                _same(got, ref, tag)
                _not_vacuous(ref, tag)
                n_checked += int(ref[1].sum())
        print(f"{preset} {prec}: {n_checked} records compared")
    finally:
        eng.close()


def test_pipeline_identity_bt709(models, frames):
    # the matrix reaches the kernel through every path: BT.709 frames against their BT.709 conversion
    eng = _engine(models, "v1", "fp16")
    try:
        nv = [f[0] for f in frames["720p"]]
        bgr = [R.nv12_to_bgr(f, "bt709") for f in nv]
        assert not np.array_equal(bgr[0], frames["720p"][0][1])
        sizes = [(720, 1280)] * 2
        rc, ref = _host_call(eng, "run_batch", bgr, sizes)
        assert rc == 0
        assert _set_fmt(eng, pixfmt=1, matrix=1) == 0
        rc, got = _host_call(eng, "run_batch", nv, sizes)
        assert rc == 0
        _same(got, ref, "bt709 run_batch")
        res = _result_buffers(eng, 2)
        rc, got = _device_call(eng, "run_batch_device", torch.from_numpy(np.stack(nv)).cuda(), 2, 720, 1280, res)
        assert rc == 0
        _same(got, ref, "bt709 run_batch_device")
        _not_vacuous(ref, "bt709")
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 3. state and graphs
def test_format_is_handle_state_across_eager_capture_replay(models, frames):
    fs = frames["720p"]
    nv, bgr = [f[0] for f in fs], [f[1] for f in fs]
    sizes, B, H, W = [(720, 1280)] * 2, 2, 720, 1280
    fresh = _engine(models, "v1", "fp16")
    try:
        rc, ref = _host_call(fresh, "run_batch", bgr, sizes)
        assert rc == 0
        _not_vacuous(ref, "fresh handle")
    finally:
        fresh.close()
    eng = _engine(models, "v1", "fp16")
    try:
        d_bgr, d_nv = torch.from_numpy(np.stack(bgr)).cuda(), torch.from_numpy(np.stack(nv)).cuda()
        res = _result_buffers(eng, B)
        for phase, (fmt, host, dev) in enumerate([(dict(), bgr, d_bgr), (dict(pixfmt=1), nv, d_nv), (dict(), bgr, d_bgr)]):
            assert _set_fmt(eng, **fmt) == 0
            for call in range(3):   # eager, capture, replay
                rc, got = _host_call(eng, "run_batch", host, sizes)
                assert rc == 0
                _same(got, ref, f"phase {phase} host call {call}")
                rc, got = _device_call(eng, "run_batch_device", dev, B, H, W, res)
                assert rc == 0
                _same(got, ref, f"phase {phase} device call {call}")
        # two NV12 layouts alternate over the SAME host array and the SAME device buffer: only the format tells the steps apart
        pitch = 1296
        packed, uv, fb, st = R.pack_frames(nv, pitch=pitch, uv_offset=pitch * H + 5 * pitch, frame_stride=0)
        tight = np.concatenate([f.ravel() for f in nv])
        n = max(packed.size, tight.size)
        host_buf = np.zeros(n, np.uint8)
        dev_buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
        layouts = [(dict(pixfmt=1), tight, nv[0].size), (dict(pixfmt=1, pitch=pitch, uv_offset=uv), packed, st)]
        for call in range(8):
            fmt, data, stride = layouts[call % 2]
            host_buf[:] = 0
            host_buf[:data.size] = data
            dev_buf.copy_(torch.from_numpy(host_buf))
            torch.cuda.synchronize()
            assert _set_fmt(eng, **fmt) == 0
            rc, got = _host_call(eng, "run_batch", [host_buf[i * stride:] for i in range(B)], sizes)
            assert rc == 0, eng.lib.lp_last_error()
            _same(got, ref, f"alternating layouts, host call {call}")
            rc, got = _device_call(eng, "run_batch_device", dev_buf, B, H, W, res)
            assert rc == 0, eng.lib.lp_last_error()
            _same(got, ref, f"alternating layouts, device call {call}")
    finally:
        eng.close()


def test_converter_is_profiled_and_timed(models, frames):
    eng = _engine(models, "v1", "fp16")
    try:
        nv = [f[0] for f in frames["720p"]]
        eng.set_input_format("nv12")
        eng.profile_next(True)
        _, _, _, timing = eng.run_batch(nv, CONF, IOU, MIN_AREA)
        recs = eng.profile_read()
        csc = [r for r in recs if r["name"] == "nv12_to_bgr"]
        assert len(csc) == 1 and csc[0]["layer"] == "csc" and recs[0] is csc[0]
        assert csc[0]["bytes"] == 4.5 * 2 * 720 * 1280 and csc[0]["flops"] == 0.0 and csc[0]["ms"] > 0.0
        assert timing.t_detection > 0.0
        eng.set_input_format("bgr")
        eng.profile_next(True)
        eng.run_batch([f[1] for f in frames["720p"]], CONF, IOU, MIN_AREA)
        assert not [r for r in eng.profile_read() if r["name"] == "nv12_to_bgr"]
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 4. errors
def test_format_errors_leave_the_handle_usable(models, frames):
    from litepi._ffi import LP_ERR_ARG
    fs = frames["640"]
    nv, bgr = [f[0] for f in fs], [f[1] for f in fs]
    sizes, B = [(640, 640)] * 3, 3
    eng = _engine(models, "v1", "fp16")
    try:
        rc, ref = _host_call(eng, "run_batch", bgr, sizes)
        assert rc == 0
        # what needs no size is refused by lp_set_input_format, and the format stays what it was (BGR)
        for bad in (dict(pixfmt=2), dict(pixfmt=-1), dict(pixfmt=1, matrix=2), dict(pixfmt=1, reserved0=1), dict(pixfmt=1, reserved=3),
                    dict(pixfmt=0, pitch=1920), dict(pixfmt=0, uv_offset=16), dict(pixfmt=0, frame_stride=1 << 21), dict(pixfmt=1, pitch=-2)):
            assert _set_fmt(eng, **bad) == LP_ERR_ARG, bad
            assert len(eng.lib.lp_last_error()) > 0
        rc, got = _host_call(eng, "run_batch", bgr, sizes)
        assert rc == 0
        _same(got, ref, "after refused formats")
        # what needs the frame size is refused by every frame-taking call, before anything is enqueued
        big = np.zeros(4 << 20, np.uint8)
        d_big = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda")
        res = _result_buffers(eng, B)
        cases = [("odd H", dict(pixfmt=1), (639, 640)), ("odd W", dict(pixfmt=1), (640, 639)), ("pitch < W", dict(pixfmt=1, pitch=638), (640, 640)),
                 ("uv_offset < pitch * H", dict(pixfmt=1, uv_offset=409599), (640, 640)),
                 ("uv_offset < pitch * H, pitched", dict(pixfmt=1, pitch=704, uv_offset=409600), (640, 640))]
        for name, fmt, (H, W) in cases:
            assert _set_fmt(eng, **fmt) == 0, name
            for entry in ("detect", "run_batch", "run_tiled"):
                rc, _ = _host_call(eng, entry, [big] * B, [(H, W)] * B)
                assert rc == LP_ERR_ARG, f"{name}: {entry} returned {rc}"
            for entry in ("run_batch_device", "run_tiled_device"):
                rc, _ = _device_call(eng, entry, d_big, B, H, W, res)
                assert rc == LP_ERR_ARG, f"{name}: {entry} returned {rc}"
        assert _set_fmt(eng, pixfmt=1, frame_stride=614399) == 0   # smaller than one frame: the device entry points refuse it
        for entry in ("run_batch_device", "run_tiled_device"):
            rc, _ = _device_call(eng, entry, d_big, B, 640, 640, res)
            assert rc == LP_ERR_ARG, f"frame_stride: {entry} returned {rc}"
        rc, got = _host_call(eng, "run_batch", nv, sizes)        # ... and host frames ignore frame_stride
        assert rc == 0
        _same(got, ref, "host frames ignore frame_stride")
        # good calls on the same handle: NV12, then BGR again
        assert _set_fmt(eng, pixfmt=1) == 0
        rc, got = _host_call(eng, "run_batch", nv, sizes)
        assert rc == 0
        _same(got, ref, "NV12 after the errors")
        rc, got = _device_call(eng, "run_batch_device", torch.from_numpy(np.stack(nv)).cuda(), B, 640, 640, res)
        assert rc == 0
        _same(got, ref, "NV12 device path after the errors")
        assert eng.lib.lp_set_input_format(eng._h, None) == 0   # NULL = packed BGR
        rc, got = _host_call(eng, "run_batch", bgr, sizes)
        assert rc == 0
        _same(got, ref, "BGR after the errors")
        _not_vacuous(ref, "errors")
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 5. Python surface
def _strip(outs):
    """what must be equal between two runs: everything but the clocks"""
    rows = []
    for res, m in outs:
        rows.append(([{k: r[k] for k in ("bbox", "det_class", "det_conf", "cls_class", "cls_conf")} for r in res],
                     m.num_detections, m.det_confidence_avg, m.cls_confidence_avg))
    return rows


@pytest.fixture(scope="module")
def cls_file(tmp_path_factory, models):
    p = str(tmp_path_factory.mktemp("pixfmt_cls") / "cls.pth")
    torch.save({k: torch.from_numpy(v) for k, v in models["cls"].items()}, p)
    return p


@pytest.mark.parametrize("tiled", [False, True], ids=["letterbox", "tiled"])
def test_hybrid_pipeline_nv12_arrays(models, frames, cls_file, tiled):
    from litepi import HybridPipeline
    p, b = models["v1"]
    fs = frames["mixed"]
    kw = dict(num_classes=91, precision="fp16", max_batch=16, max_det=300, tile_overlap=128 if tiled else None)
    ref_pipe = HybridPipeline(p, b, cls_file, "shufflenetv2", **kw)
    try:
        ref = _strip(ref_pipe.run_batch([f[1] for f in fs], CONF, IOU, MIN_AREA))
        ref_one = _strip([ref_pipe.run(fs[1][1], CONF, IOU, MIN_AREA)])
    finally:
        ref_pipe.close()
    pipe = HybridPipeline(p, b, cls_file, "shufflenetv2", pixel_format="nv12", csc_matrix="bt601", **kw)
    try:
        assert fs[1][0].shape == (1080, 1280)
        assert _strip(pipe.run_batch([f[0] for f in fs], CONF, IOU, MIN_AREA)) == ref
        assert _strip([pipe.run(fs[1][0], CONF, IOU, MIN_AREA)]) == ref_one
        with pytest.raises(ValueError):   # never a silent BGR interpretation
            pipe.run(fs[1][1], CONF, IOU, MIN_AREA)
    finally:
        pipe.close()
    assert sum(len(r[0]) for r in ref) >= 1 and any(d["cls_class"] >= 0 for r in ref for d in r[0])


def test_hybrid_pipeline_lanes_refuse_nv12(models, cls_file, monkeypatch):
    from litepi import HybridPipeline
    monkeypatch.setenv("LITEPI_DROPIN_LANES", "2")
    with pytest.raises(ValueError, match="LITEPI_DROPIN_LANES"):
        HybridPipeline(*models["v1"], cls_file, "shufflenetv2", num_classes=91, max_batch=8, pixel_format="nv12")


def test_e2e_raw_frames_equals_images(models, frames, cls_file, tmp_path, capsys):
    import pandas as pd
    from PIL import Image
    from litepi import e2e
    p, b = models["v1"]
    fs = frames["720p"] + frames["720p"][:1]
    rng = np.random.default_rng(6)
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir(); lab_dir.mkdir()
    with open(tmp_path / "clip.nv12", "wb") as f:
        for i, (nv, bgr) in enumerate(fs):
            f.write(nv.tobytes())
            Image.fromarray(bgr[:, :, ::-1]).save(img_dir / f"frame_{i + 1:06d}.png")
            if i != 1:   # a frame without a label file has no boxes, like an image
                with open(lab_dir / f"frame_{i + 1:06d}.txt", "w") as g:
                    for _ in range(3):
                        xc, yc, w, h = rng.uniform(0.2, 0.8), rng.uniform(0.2, 0.8), rng.uniform(0.05, 0.2), rng.uniform(0.05, 0.2)
                        g.write(f"{int(rng.integers(0, 91))} {xc:.6f} {yc:.6f} {w:.6f} {h:.6f}\n")
    classes = tmp_path / "idx2label.json"
    classes.write_text(json.dumps({str(i): f"sign_{i}" for i in range(91)}))
    common = ["--detector_param", p, "--detector_bin", b, "--classifier", cls_file, "--clf_arch", "shufflenetv2", "--labels", str(lab_dir),
              "--classes", str(classes), "--batch_images", "2", "--max_det", "300", "--yolo_conf", "0.25"]
    out_img, out_raw = tmp_path / "out_img", tmp_path / "out_raw"
    assert e2e.main(common + ["--input", str(img_dir), "--output", str(out_img)]) == 0
    assert e2e.main(common + ["--raw_frames", str(tmp_path / "clip.nv12"), "--frame_size", "1280x720", "--pixel_format", "nv12",
                              "--output", str(out_raw), "--save_viz", "1"]) == 0
    capsys.readouterr()
    a, r = pd.read_csv(out_img / "comparison_summary.csv"), pd.read_csv(out_raw / "comparison_summary.csv")
    assert len(a) == len(r) == 1 and a.loc[0, "num_test_images"] == 3
    same = [c for c in a.columns if c != "fps"]   # (the clock is the one column that cannot repeat)
    assert a[same].equals(r[same]), f"{a[same].to_dict()} vs {r[same].to_dict()}"
    viz = sorted((out_raw / a.loc[0, "model_combination"] / "visualizations").glob("vis_frame_*.png"))
    assert [v.name for v in viz] == ["vis_frame_000001.png", "vis_frame_000002.png", "vis_frame_000003.png"]
    assert Image.open(viz[0]).size == (1280, 720)
    with open(tmp_path / "clip.nv12", "ab") as f:   # a trailing partial frame is an error
        f.write(b"\x00" * 100)
    with pytest.raises(ValueError, match="whole number"):
        e2e.main(common + ["--raw_frames", str(tmp_path / "clip.nv12"), "--frame_size", "1280x720", "--pixel_format", "nv12",
                           "--output", str(tmp_path / "out_bad")])
