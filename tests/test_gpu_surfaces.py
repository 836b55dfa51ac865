"""GPU tests of decoder surfaces in place (include/litepi.h lp_surface), everything through the C-ABI.  Surfaces are
torch device tensors: every frame its own allocations, luma and chroma apart, a pitch and an address offset per plane.

1. the converter alone (lp_test_convert_surfaces) is bit-exact against the int64 oracle of tests/pixfmt_ref.py, NV12 and P010;
2. lp_run_surfaces_device / lp_run_views_surfaces_device give byte for byte what lp_run_batch_device / lp_run_views_device give on
   the BGR frames the oracle makes from the surfaces;
3. the captured step replays while the surfaces' addresses and pitches move, with no host synchronise between the calls;
4. every argument error is LP_ERR_ARG with nothing enqueued, and the handle (and its lp_set_input_format state) stays usable;
5. tracker and inventory behind the surfaces call give what they give behind lp_run_batch_device on the converted frames.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pixfmt_ref as R
import surface_ref as S

pytestmark = pytest.mark.gpu

CONF, IOU, MIN_AREA = 0.25, 0.45, 50
OFFSETS = {"nv12": (0, 1, 3, 8, 16), "p010": (0, 2, 6, 16)}


# ---------------------------------------------------------------------------- surfaces out of host frames
def _dev_plane(rows, pitch=0, offset=0):
    """[n, W] samples -> a strided 2-D device view (uint8, or int16 for uint16 samples) `offset` bytes into an allocation of
    its own, rows `pitch` bytes apart; the allocation ends with the last row's samples"""
    buf, off = S.pack_plane(rows, pitch=pitch, offset=offset)
    t = torch.from_numpy(buf).cuda()
    n, w = rows.shape
    if rows.dtype == np.uint16:
        assert off % 2 == 0 and pitch % 2 == 0
        return t.view(torch.int16).as_strided((n, w), ((pitch // 2) or w, 1), off // 2)
    return t.as_strided((n, w), (pitch or w, 1), off)


def _surface(frame, pitch_y=0, pitch_uv=0, off_y=0, off_uv=0):
    """tight frame [H * 3 // 2, W] (uint8: NV12, uint16: P010) -> (Surface, pixfmt, the tensors that keep it alive)"""
    from litepi.surfaces import surface_from_tensors
    y, uv = S.split_planes(frame)
    ty, tuv = _dev_plane(y, pitch_y, off_y), _dev_plane(uv, pitch_uv, off_uv)
    s, fmt = surface_from_tensors(ty, tuv)
    assert (s.pitch_y, s.pitch_uv) == (pitch_y or y.shape[1] * frame.itemsize, pitch_uv or y.shape[1] * frame.itemsize)
    return s, fmt, (ty, tuv)


def _as_format(frame, fmt, rng):
    return S.widen(frame, rng=rng) if fmt == "p010" else frame


def _pool(frames, fmt, rng, round_to=256, off_y=0, off_uv=0, extra=0):
    """one surface per tight NV12 frame, as a decoder pool hands them out: pitches rounded up to `round_to` (+ extra)"""
    surfaces, keep = [], []
    for f in frames:
        bps = S.SAMPLE_BYTES[fmt]
        W = f.shape[1]
        p = -(-W * bps // round_to) * round_to + extra
        s, got, t = _surface(_as_format(f, fmt, rng), p, p + round_to, off_y, off_uv)
        assert got == fmt
        surfaces.append(s)
        keep.append(t)
    return surfaces, keep


# ---------------------------------------------------------------------------- 1. the converter
@pytest.fixture(scope="module")
def conv_eng():
    from litepi import Engine
    e = Engine(precision="fp16", max_batch=64, max_det=8, num_classes=4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def all_yuv():
    frames = R.all_yuv_frames()
    return frames, {m: [R.nv12_to_bgr(f, m) for f in frames] for m in ("bt601", "bt709")}


@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_converter_all_2_24_inputs(conv_eng, all_yuv, fmt, matrix):
    frames, want = all_yuv
    rng = np.random.default_rng(5)
    surfaces, keep = [], []
    for i, f in enumerate(frames):   # every frame its own two allocations; a third of them tight and aligned
        bps = S.SAMPLE_BYTES[fmt]
        s, got, t = _surface(_as_format(f, fmt, rng), (0, 512 * bps + 16, 1024 * bps + 2)[i % 3], (0, 1024 * bps, 512 * bps + 6)[i % 3],
                             OFFSETS[fmt][i % len(OFFSETS[fmt])] if i % 3 else 0, OFFSETS[fmt][(i + 1) % len(OFFSETS[fmt])] if i % 3 else 0)
        assert got == fmt
        surfaces.append(s)
        keep.append(t)
    got = conv_eng.test_convert_surfaces(surfaces, fmt, matrix)
    for i in range(len(frames)):
        assert np.array_equal(got[i], want[matrix][i]), f"{fmt} {matrix}: frame {i} differs in {int((got[i] != want[matrix][i]).sum())} bytes"


SIZES = [(2, 2), (2, 16), (6, 18), (34, 50), (270, 1920)]


def _pitches(W, fmt):
    row = W * S.SAMPLE_BYTES[fmt]
    return [p for p in (row, row + 2, 1936, 2048) if p >= row]


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
def test_converter_sizes_pitches_and_addresses(conv_eng, fmt, B, H, W):
    rng = np.random.default_rng(H * 7 + W + B)
    frames = [rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8) for _ in range(B)]
    want = [R.nv12_to_bgr(f, "bt601") for f in frames]
    pitches, offs = _pitches(W, fmt), OFFSETS[fmt]
    n = 0
    for pi, pitch in enumerate(pitches):
        pitch_uv = pitches[(pi + 1) % len(pitches)]   # the two planes' pitches are unequal wherever two pitches fit
        for oi, off in enumerate(offs):
            surfaces, keep = [], []
            for i, f in enumerate(frames):   # frame i's chroma plane sits at another offset than its luma plane
                s, got, t = _surface(_as_format(f, fmt, rng), pitch, pitch_uv, off, offs[(oi + 1 + i) % len(offs)])
                surfaces.append(s)
                keep.append(t)
            got = conv_eng.test_convert_surfaces(surfaces, fmt, "bt601")   # (the hook itself checks its guard bytes)
            for i in range(B):
                assert np.array_equal(got[i], want[i]), \
                    f"{fmt} {W}x{H} frame {i} of {B}, pitches {pitch}/{pitch_uv}, offset {off}: {int((got[i] != want[i]).sum())} bytes differ"
            n += 1
    assert n == len(pitches) * len(offs) and len(pitches) >= 2


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("matrix", ["bt601", "bt709"])
def test_converter_three_sizes_in_one_call(conv_eng, fmt, matrix):
    rng = np.random.default_rng(77)
    sizes = [(270, 1920), (6, 18), (34, 50), (2, 16), (64, 64)]   # the largest first: later frames leave grid blocks idle
    frames = [rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for h, w in sizes]
    surfaces, keep = [], []
    for i, f in enumerate(frames):
        bps = S.SAMPLE_BYTES[fmt]
        aligned = i in (0, 4)   # (1920 and 64 wide, aligned planes and pitches: the aligned path next to the others)
        s, _, t = _surface(_as_format(f, fmt, rng), 0 if aligned else f.shape[1] * bps + 2 * i, 2048 * bps if aligned else 0,
                           0 if aligned else OFFSETS[fmt][i % 4], 0 if aligned else OFFSETS[fmt][(i + 2) % 4])
        surfaces.append(s)
        keep.append(t)
    got = conv_eng.test_convert_surfaces(surfaces, fmt, matrix)
    for i, f in enumerate(frames):
        want = R.nv12_to_bgr(f, matrix)
        assert got[i].shape == want.shape and np.array_equal(got[i], want), f"{fmt} {matrix}: frame {i} {sizes[i]} differs"


# ---------------------------------------------------------------------------- models and frames of the pipeline tests
def _noise_nv12(rng, H, W):
    """an NV12 frame made with the forward helper from BGR noise, and its BGR conversion"""
    nv = R.bgr_to_nv12(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    return nv, R.nv12_to_bgr(nv, "bt601")


@pytest.fixture(scope="module")
def frames():
    rng = np.random.default_rng(2024)
    sets = {"640": [_noise_nv12(rng, 640, 640) for _ in range(3)],          # the no-letterbox path
            "720p": [_noise_nv12(rng, 720, 1280) for _ in range(2)]}
    sets["mixed"] = [sets["640"][0], sets["720p"][1], _noise_nv12(rng, 482, 366)]   # (366 is not a multiple of 16)
    return sets


def _shift_bias(p, b, every, det_input):
    """the bias-shift recipe of test_gpu_pixfmt.py's models fixture: on EVERY frame at least three anchors pass conf 0.25 with a
    margin of 0.1 in the logit, measured with the device's own scores on the letterboxed BGR frames"""
    from litepi import Engine, ncnn_export
    e = Engine(precision="fp16", max_batch=len(every), max_det=300, num_classes=91, det_input=det_input)
    try:
        e.load_detector(p, b)
        lb = np.stack([e.test_letterbox(f)[0] for f in every])
        s = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64), axis=1)[:, ::-1]
    finally:
        e.close()
    third = s[:, 2].min()
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - (np.log(third / (1 - third)) - 0.1)))


@pytest.fixture(scope="module")
def models(tmp_path_factory, frames):
    """seeded v1 / v2 detectors (and v1 for a 384 x 640 input) with the class bias shifted so that something is found on every frame"""
    from litepi import ncnn_export
    from litepi.backend import random_shufflenet_state
    d = tmp_path_factory.mktemp("surface_models")
    out = {"cls": random_shufflenet_state(91, seed=3)}
    every = [bgr for s in ("640", "720p", "mixed") for _, bgr in frames[s]]
    for preset in ("v1", "v2"):
        p, b = str(d / f"{preset}.param"), str(d / f"{preset}.bin")
        ncnn_export.export_detector(p, b, preset, seed=4321, cls_bias=0.0)
        _shift_bias(p, b, every, 640)
        out[preset] = (p, b)
    p, b = str(d / "rect.param"), str(d / "rect.bin")
    ncnn_export.export_detector(p, b, "v1", seed=4321, cls_bias=0.0, size=(384, 640))
    _shift_bias(p, b, [bgr for _, bgr in frames["720p"]], (384, 640))
    out["rect"] = (p, b)
    return out


def _engine(models, preset, prec, max_batch=16, classifier=True, det_input=640):
    from litepi import Engine
    e = Engine(precision=prec, max_batch=max_batch, max_det=300, num_classes=91, det_input=det_input)
    e.load_detector(*models[preset])
    if classifier:
        e.load_classifier(models["cls"])
    return e


def _result_buffers(eng, B):
    return (torch.zeros(B * eng.cfg.max_det * 32, dtype=torch.uint8, device="cuda"), torch.zeros(3 * B, dtype=torch.int32, device="cuda"))


def _unpack(eng, dd, dc, B):
    """device records and counts -> (records per frame as bytes, kept, pre-filter counts, mean-score bits)"""
    from litepi._ffi import DET_DTYPE
    cnt = dc.cpu().numpy()
    dets = dd.cpu().numpy().view(DET_DTYPE).reshape(-1, eng.cfg.max_det)
    kept = cnt[:B].astype(np.int64)
    return ([dets[i, :kept[i]].tobytes() for i in range(B)], kept, cnt[B:2 * B].astype(np.int64), cnt[2 * B:3 * B].view(np.uint32).copy(),
            dets.copy())


def _read(eng, res, B):
    eng.synchronize()
    torch.cuda.synchronize()
    return _unpack(eng, res[0], res[1], B)


def _ref_batch(eng, bgr, res, views=None):
    B, (H, W) = len(bgr), bgr[0].shape[:2]
    x = torch.from_numpy(np.stack(bgr)).cuda()
    if views is None:
        eng.run_batch_device(x.data_ptr(), B, H, W, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr())
    else:
        eng.run_views_device(x.data_ptr(), B, H, W, views, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr())
    return _read(eng, res, B)


def _run_surfaces(eng, surfaces, fmt, res, views=None, matrix="bt601"):
    if views is None:
        eng.run_surfaces_device(surfaces, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr(), pixfmt=fmt, matrix=matrix)
    else:
        eng.run_views_surfaces_device(surfaces, views, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr(), pixfmt=fmt, matrix=matrix)
    return _read(eng, res, len(surfaces))


def _same(a, b, tag):
    assert np.array_equal(a[1], b[1]), f"{tag}: kept counts differ ({a[1]} vs {b[1]})"
    assert a[0] == b[0], f"{tag}: records differ"
    assert np.array_equal(a[2], b[2]), f"{tag}: pre-filter counts differ"
    assert np.array_equal(a[3], b[3]), f"{tag}: mean score bits differ"


def _not_vacuous(r, tag):
    assert int(r[1].sum()) >= 1, f"{tag}: no kept box, the comparison is empty"
    n_cls = sum(int((r[4][i, :r[1][i]]["cls_class"] >= 0).sum()) for i in range(len(r[1])))
    assert n_cls >= 1, f"{tag}: no classified ROI, the comparison is empty"


def _host_run_batch(eng, imgs):
    """lp_run_batch on host BGR frames of individual sizes, in the shape of _unpack"""
    from litepi._ffi import DET_DTYPE, LpTiming
    B = len(imgs)
    keep = [np.ascontiguousarray(b, dtype=np.uint8) for b in imgs]
    ptrs = (C.c_void_p * B)(*[k.ctypes.data for k in keep])
    hs = (C.c_int * B)(*[k.shape[0] for k in keep])
    ws = (C.c_int * B)(*[k.shape[1] for k in keep])
    dets = np.zeros((B, eng.cfg.max_det), dtype=DET_DTYPE)
    counts, num_det, avg, timing = (C.c_int * B)(), (C.c_int * B)(), (C.c_float * B)(), LpTiming()
    rc = eng.lib.lp_run_batch(eng._h, ptrs, hs, ws, B, CONF, IOU, MIN_AREA, dets.ctypes.data, counts, num_det, avg, C.byref(timing))
    assert rc == 0, eng.lib.lp_last_error()
    cnt = np.array(counts[:], dtype=np.int64)
    return ([dets[i, :cnt[i]].tobytes() for i in range(B)], cnt, np.array(num_det[:], dtype=np.int64),
            np.array(avg[:], dtype=np.float32).view(np.uint32), dets)


# ---------------------------------------------------------------------------- 2. pipeline equality
VIEWS = ["full", (100, 40, 640, 600)]


@pytest.mark.parametrize("preset", ["v1", "v2"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_pipeline_equality_surfaces_vs_converted_bgr(models, frames, preset, prec):
    eng = _engine(models, preset, prec)
    rng = np.random.default_rng(31)
    n_checked = 0
    try:
        for set_name in ("640", "720p"):
            nv, bgr = [f[0] for f in frames[set_name]], [f[1] for f in frames[set_name]]
            B = len(nv)
            res = _result_buffers(eng, B)
            ref = _ref_batch(eng, bgr, res)
            _not_vacuous(ref, f"{preset} {prec} {set_name}")
            ref_views = _ref_batch(eng, bgr, res, VIEWS) if set_name == "720p" else None
            for fmt, off_y, off_uv, extra in (("nv12", 0, 0, 0), ("nv12", 3, 8, 2), ("p010", 0, 0, 0), ("p010", 6, 2, 2)):
                surfaces, keep = _pool(nv, fmt, rng, off_y=off_y, off_uv=off_uv, extra=extra)
                tag = f"{preset} {prec} {set_name} {fmt} offsets {off_y}/{off_uv}"
                res[0].zero_(); res[1].zero_()
                _same(_run_surfaces(eng, surfaces, fmt, res), ref, tag)
                n_checked += int(ref[1].sum())
                if ref_views is not None:
                    res[0].zero_(); res[1].zero_()
                    _same(_run_surfaces(eng, surfaces, fmt, res, VIEWS), ref_views, tag + " views")
                    n_checked += int(ref_views[1].sum())
        # surfaces of individual sizes in one call against lp_run_batch on the converted host frames
        nv, bgr = [f[0] for f in frames["mixed"]], [f[1] for f in frames["mixed"]]
        ref = _host_run_batch(eng, bgr)
        _not_vacuous(ref, f"{preset} {prec} mixed")
        res = _result_buffers(eng, 3)
        for fmt in ("nv12", "p010"):
            surfaces, keep = _pool(nv, fmt, rng, round_to=64, off_y=OFFSETS[fmt][1], off_uv=OFFSETS[fmt][2])
            _same(_run_surfaces(eng, surfaces, fmt, res), ref, f"{preset} {prec} mixed sizes {fmt}")
            n_checked += int(ref[1].sum())
        print(f"{preset} {prec}: {n_checked} records compared")
    finally:
        eng.close()


def test_bt709_reaches_the_kernel_through_the_pipeline(models, frames):
    eng = _engine(models, "v1", "fp16")
    try:
        nv = [f[0] for f in frames["720p"]]
        bgr = [R.nv12_to_bgr(f, "bt709") for f in nv]
        assert not np.array_equal(bgr[0], frames["720p"][0][1])
        res = _result_buffers(eng, 2)
        ref = _ref_batch(eng, bgr, res)
        _not_vacuous(ref, "bt709")
        for fmt in ("nv12", "p010"):
            surfaces, keep = _pool(nv, fmt, np.random.default_rng(1))
            _same(_run_surfaces(eng, surfaces, fmt, res, matrix="bt709"), ref, f"bt709 {fmt}")
    finally:
        eng.close()


def test_rectangular_handle(models, frames):
    from litepi._ffi import LP_ERR_STATE, LitepiError
    eng = _engine(models, "rect", "fp16", max_batch=4, det_input=(384, 640))
    try:
        nv, bgr = [f[0] for f in frames["720p"]], [f[1] for f in frames["720p"]]
        res = _result_buffers(eng, 2)
        ref = _ref_batch(eng, bgr, res)
        _not_vacuous(ref, "384x640 handle")
        for fmt in ("nv12", "p010"):
            surfaces, keep = _pool(nv, fmt, np.random.default_rng(2))
            for call in range(3):   # eager, capture, replay
                res[0].zero_(); res[1].zero_()
                _same(_run_surfaces(eng, surfaces, fmt, res), ref, f"384x640 handle {fmt} call {call}")
            before = eng.graph_stats()
            with pytest.raises(LitepiError) as ei:
                eng.run_views_surfaces_device(surfaces, VIEWS, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr(), pixfmt=fmt)
            assert ei.value.code == LP_ERR_STATE and "384x640" in str(ei.value) and "square" in str(ei.value)
            with pytest.raises(LitepiError) as twin:
                eng.run_views_device(keep[0][0].data_ptr(), 2, 720, 1280, VIEWS, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr())
            assert twin.value.code == LP_ERR_STATE   # the same check, the same message but for the entry point's name
            assert str(ei.value).replace("lp_run_views_surfaces_device", "lp_run_views_device") == str(twin.value)
            assert eng.graph_stats() == before
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 3. the step replays while the pointers move
@pytest.mark.parametrize("entry", ["batch", "views"])
def test_step_replays_while_the_pointers_move(models, frames, entry):
    views = VIEWS if entry == "views" else None
    fs = frames["720p"] if entry == "views" else frames["640"]
    nv, bgr = [f[0] for f in fs], [f[1] for f in fs]
    # two pools at different addresses and pitches that hold different frames of one size
    pool_frames = [[nv[0], nv[1]], [nv[1], nv[0]]]
    pool_bgr = [[bgr[0], bgr[1]], [bgr[1], bgr[0]]]
    B, N = 2, 12
    eng = _engine(models, "v1", "fp16")
    st = torch.cuda.Stream()
    try:
        res = _result_buffers(eng, B)
        refs = [_ref_batch(eng, pool_bgr[k], res, views) for k in range(2)]
        _not_vacuous(refs[0], entry)
        assert refs[0][0] != refs[1][0], "the pools' results must differ for the test to tell them apart"
        rng = np.random.default_rng(8)
        pools = [_pool(pool_frames[0], "nv12", rng, round_to=256), _pool(pool_frames[1], "nv12", rng, round_to=64, off_y=8, off_uv=3, extra=2)]
        assert pools[0][0][0].pitch_y != pools[1][0][0].pitch_y and pools[0][0][0].y_ptr != pools[1][0][0].y_ptr
        out_d = [torch.zeros_like(res[0]) for _ in range(N)]
        out_c = [torch.zeros_like(res[1]) for _ in range(N)]
        stats = []
        torch.cuda.synchronize()
        eng.set_stream(st.cuda_stream)
        before = eng.graph_stats()
        with torch.cuda.stream(st):
            for k in range(N):   # no host synchronise between the calls: only stream order keeps the tables apart
                surfaces = pools[k % 2][0]
                if views is None:
                    eng.run_surfaces_device(surfaces, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr())
                else:
                    eng.run_views_surfaces_device(surfaces, views, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr())
                out_d[k].copy_(res[0], non_blocking=True)
                out_c[k].copy_(res[1], non_blocking=True)
                stats.append(eng.graph_stats())
        st.synchronize()
        for k in range(N):
            _same(_unpack(eng, out_d[k], out_c[k], B), refs[k % 2], f"{entry} call {k} (pool {k % 2})")
        delta = [{key: s[key] - before[key] for key in s} for s in stats]
        assert delta[0] == dict(entries=1, eager=1, captures=0, replays=0), delta[0]
        assert delta[1] == dict(entries=1, eager=1, captures=1, replays=0), delta[1]
        for k in range(2, N):   # replays from the third call on: one entry, one capture, whatever the surfaces' addresses
            assert delta[k] == dict(entries=1, eager=1, captures=1, replays=k - 1), (k, delta[k])
    finally:
        eng.set_stream(0)
        eng.close()


def test_formats_alternate_on_one_handle(models, frames):
    nv, bgr = [f[0] for f in frames["640"]], [f[1] for f in frames["640"]]
    eng = _engine(models, "v1", "fp16")
    try:
        res = _result_buffers(eng, 3)
        ref = _ref_batch(eng, bgr, res)
        _not_vacuous(ref, "formats")
        rng = np.random.default_rng(9)
        pools = {"nv12": _pool(nv, "nv12", rng), "p010": _pool(nv, "p010", rng)}
        before = eng.graph_stats()
        seen = []
        for phase, fmt in enumerate(["nv12", "p010", "nv12"]):
            for call in range(3):
                res[0].zero_(); res[1].zero_()
                _same(_run_surfaces(eng, pools[fmt][0], fmt, res), ref, f"phase {phase} ({fmt}) call {call}")
                s = eng.graph_stats()
                seen.append({k: s[k] - before[k] for k in s})
        # a format's first two calls are eager and capture, whatever the other format has captured; its later calls replay its own step
        assert [s["eager"] for s in seen] == [1, 1, 1, 2, 2, 2, 2, 2, 2]
        assert [s["captures"] for s in seen] == [0, 1, 1, 1, 2, 2, 2, 2, 2]
        assert [s["replays"] for s in seen] == [0, 0, 1, 1, 1, 2, 3, 4, 5]
        assert seen[-1]["entries"] == 2
    finally:
        eng.close()


def test_converter_is_profiled(models, frames):
    eng = _engine(models, "v1", "fp16")
    try:
        nv = [f[0] for f in frames["720p"]]
        res = _result_buffers(eng, 2)
        for fmt, name, per_pixel in (("nv12", "surfaces_to_bgr", 4.5), ("p010", "surfaces_to_bgr_p010", 6.0)):
            surfaces, keep = _pool(nv, fmt, np.random.default_rng(3))
            eng.profile_next(True)
            _run_surfaces(eng, surfaces, fmt, res)
            recs = eng.profile_read()
            csc = [r for r in recs if r["layer"] == "csc"]
            assert len(csc) == 1 and csc[0]["name"] == name and recs[0] is csc[0]
            assert csc[0]["bytes"] == per_pixel * 2 * 720 * 1280 and csc[0]["ms"] > 0.0
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 4. errors
def _raw_call(eng, entry, fmt, recs, B, res, null_fmt=False, null_surfaces=False, views=VIEWS):
    """the entry points on raw field values (no Python-side validation) -> status"""
    from litepi import _ffi
    f = _ffi.LpSurfaceFormat()
    for k, v in fmt.items():
        if k == "reserved":
            f.reserved[v] = 1
        else:
            setattr(f, k, v)
    arr = (_ffi.LpSurface * max(1, len(recs)))()
    for rec, s in zip(arr, recs):
        rec.plane[0], rec.plane[1] = s["y"], s["uv"]
        rec.pitch[0], rec.pitch[1] = s["pitch_y"], s["pitch_uv"]
        rec.height, rec.width = s["h"], s["w"]
        if "reserved" in s:
            rec.reserved[s["reserved"]] = 1
    fp, sp = (None if null_fmt else C.byref(f)), (None if null_surfaces else arr)
    dd, dc = C.c_void_p(res[0].data_ptr()), C.c_void_p(res[1].data_ptr())
    if entry == "batch":
        return eng.lib.lp_run_surfaces_device(eng._h, fp, sp, B, CONF, IOU, MIN_AREA, dd, dc)
    v = np.array([[-1, -1, -1, -1] if w == "full" else list(w) for w in views], np.int32)
    return eng.lib.lp_run_views_surfaces_device(eng._h, fp, sp, B, v.ctypes.data_as(C.POINTER(C.c_int)), len(v), CONF, IOU, MIN_AREA, dd, dc)


def test_argument_errors_enqueue_nothing_and_leave_the_handle_usable(models, frames):
    from litepi._ffi import LP_ERR_ARG
    nv, bgr = [f[0] for f in frames["720p"]], [f[1] for f in frames["720p"]]
    B = 2
    eng = _engine(models, "v1", "fp16", max_batch=4)
    try:
        res = _result_buffers(eng, 4)
        ref = {None: _ref_batch(eng, bgr, res), "views": _ref_batch(eng, bgr, res, VIEWS)}
        _not_vacuous(ref[None], "errors")
        rng = np.random.default_rng(10)
        pools = {fmt: _pool(nv, fmt, rng) for fmt in ("nv12", "p010")}

        def recs(fmt, **change):
            out = [dict(y=s.y_ptr, uv=s.uv_ptr, pitch_y=s.pitch_y, pitch_uv=s.pitch_uv, h=s.height, w=s.width) for s in pools[fmt][0]]
            which = change.pop("which", 1)
            out[which].update(change)
            return out

        NV, P = dict(pixfmt=1), dict(pixfmt=2)
        cases = [("null fmt", NV, recs("nv12"), B, dict(null_fmt=True)), ("null surfaces", NV, recs("nv12"), B, dict(null_surfaces=True)),
                 ("pixfmt 0", dict(pixfmt=0), recs("nv12"), B, {}), ("pixfmt 3", dict(pixfmt=3), recs("nv12"), B, {}),
                 ("matrix 2", dict(pixfmt=1, matrix=2), recs("nv12"), B, {}), ("format reserved", dict(pixfmt=1, reserved=2), recs("nv12"), B, {}),
                 ("surface reserved", NV, recs("nv12", reserved=0), B, {}), ("B = 0", NV, recs("nv12"), 0, {}),
                 ("B > max_batch", NV, recs("nv12") * 3, 5, {}), ("null luma", NV, recs("nv12", y=0), B, {}),
                 ("null chroma", P, recs("p010", uv=0, which=0), B, {}), ("odd height", NV, recs("nv12", h=719), B, {}),
                 ("odd width", NV, recs("nv12", w=1279), B, {}), ("zero height", NV, recs("nv12", h=0), B, {}),
                 ("negative width", NV, recs("nv12", w=-1280), B, {}), ("NV12 luma pitch < W", NV, recs("nv12", pitch_y=1278), B, {}),
                 ("NV12 chroma pitch < W", NV, recs("nv12", pitch_uv=640), B, {}), ("P010 luma pitch < 2 W", P, recs("p010", pitch_y=1280), B, {}),
                 ("P010 chroma pitch < 2 W", P, recs("p010", pitch_uv=2558), B, {}), ("negative pitch", NV, recs("nv12", pitch_uv=-1536), B, {}),
                 ("P010 odd luma address", P, recs("p010", y=pools["p010"][0][1].y_ptr + 1), B, {}),
                 ("P010 odd chroma address", P, recs("p010", uv=pools["p010"][0][1].uv_ptr + 3), B, {}),
                 ("P010 odd luma pitch", P, recs("p010", pitch_y=2561), B, {}), ("P010 odd chroma pitch", P, recs("p010", pitch_uv=2817), B, {})]
        res[0].fill_(0x5A); res[1].fill_(0x5A5A5A5A)
        torch.cuda.synchronize()
        before = eng.graph_stats()
        for name, fmt, rr, b, kw in cases:
            for entry in ("batch", "views"):
                rc = _raw_call(eng, entry, fmt, rr, b, res, **kw)
                assert rc == LP_ERR_ARG, f"{name}: {entry} returned {rc}"
                assert len(eng.lib.lp_last_error()) > 0
        # the views variant alone: unequal sizes (fine for the plain call, which the good call below shows on mixed sizes), bad views
        assert _raw_call(eng, "views", NV, recs("nv12", h=718), B, res) == LP_ERR_ARG
        assert _raw_call(eng, "views", NV, recs("nv12"), B, res, views=["full", (900, 40, 640, 600)]) == LP_ERR_ARG
        assert _raw_call(eng, "views", NV, recs("nv12"), B, res, views=["full", (0, 0, 320, 320), (100, 40, 640, 600)]) == LP_ERR_ARG   # 6 > max_batch
        eng.synchronize()
        torch.cuda.synchronize()
        assert eng.graph_stats() == before, "a refused call ran or captured a step"
        assert bool((res[0] == 0x5A).all()) and bool((res[1] == 0x5A5A5A5A).all()), "a refused call wrote results"
        # good calls on the same handle
        for fmt in ("nv12", "p010"):
            _same(_run_surfaces(eng, pools[fmt][0], fmt, res), ref[None], f"{fmt} after the errors")
            _same(_run_surfaces(eng, pools[fmt][0], fmt, res, VIEWS), ref["views"], f"{fmt} views after the errors")
    finally:
        eng.close()


def test_input_format_state_is_neither_read_nor_changed(models, frames):
    nv, bgr = [f[0] for f in frames["640"]], [f[1] for f in frames["640"]]
    eng = _engine(models, "v1", "fp16")
    try:
        res = _result_buffers(eng, 3)
        ref = _ref_batch(eng, bgr, res)
        _not_vacuous(ref, "state")
        eng.set_input_format("nv12", "bt709")   # another matrix than the surfaces call's: it must not leak either way
        ref709 = [R.nv12_to_bgr(f, "bt709") for f in nv]
        d_nv = torch.from_numpy(np.stack(nv)).cuda()
        surfaces, keep = _pool(nv, "p010", np.random.default_rng(4))
        for call in range(3):
            res[0].zero_(); res[1].zero_()
            _same(_run_surfaces(eng, surfaces, "p010", res, matrix="bt601"), ref, f"surfaces call {call} on an NV12 handle")
            res[0].zero_(); res[1].zero_()
            eng.run_batch_device(d_nv.data_ptr(), 3, 640, 640, CONF, IOU, MIN_AREA, res[0].data_ptr(), res[1].data_ptr())
            got = _read(eng, res, 3)
            eng.set_input_format("bgr")
            want = _ref_batch(eng, ref709, res)
            eng.set_input_format("nv12", "bt709")
            _same(got, want, f"contiguous NV12 batch after surfaces call {call}")
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 5. neighbours
def test_tracker_and_inventory_behind_surfaces(models, frames):
    from litepi._ffi import TRACK_DTYPE
    f0 = frames["640"][0][0]
    rolled = np.concatenate([np.roll(f0[:640], 2, axis=1), np.roll(f0[640:], 2, axis=1)])   # 2 pixels right: one chroma pair
    seq = [f0, f0, rolled, f0]   # one stream, four frames
    tcfg, icfg = dict(n_streams=1, max_tracks=256, max_age=1, min_hits=2, iou_match=0.5), dict(best="area")
    sid = np.zeros(1, np.int32)
    out = {}
    for mode in ("bgr", "nv12", "p010"):
        eng = _engine(models, "v1", "fp16", max_batch=2)
        try:
            eng.tracker_create(**tcfg)
            eng.inventory_create(**icfg)
            d, c = _result_buffers(eng, 1)
            t = torch.zeros(300 * 32, dtype=torch.uint8, device="cuda")
            rng = np.random.default_rng(12)
            tracks, recs = [], []
            for k, f in enumerate(seq):
                if mode == "bgr":
                    x = torch.from_numpy(R.nv12_to_bgr(f, "bt601")[None]).cuda()
                    eng.run_batch_device(x.data_ptr(), 1, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
                else:   # every frame in a surface of its own, as a decoder pool rotates them
                    surfaces, keep = _pool([f], mode, rng, off_y=8 * (k % 2), extra=32 * (k % 3))
                    eng.run_surfaces_device(surfaces, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr(), pixfmt=mode)
                eng.track_device(d.data_ptr(), c.data_ptr(), 1, t.data_ptr(), sid)
                eng.inventory_device(d.data_ptr(), c.data_ptr(), t.data_ptr(), 1, sid, crops=True)
                eng.synchronize()
                torch.cuda.synchronize()
                n = int(c.cpu().numpy()[0])
                recs.append(d.cpu().numpy()[:n * 32].tobytes())
                tracks.append(t.cpu().numpy().view(TRACK_DTYPE)[:n].copy())
            eng.inventory_flush()
            signs, crops, dropped = eng.inventory_drain(crops=True)
            out[mode] = (recs, tracks, signs, crops, dropped)
        finally:
            eng.close()
    recs, tracks, signs, crops, dropped = out["bgr"]
    assert sum(len(t) for t in tracks) >= 4 and max(int(t["hits"].max()) for t in tracks if len(t)) >= 2, "no track lived two frames"
    assert len(signs) >= 1 and crops is not None
    for mode in ("nv12", "p010"):
        r2, t2, s2, c2, d2 = out[mode]
        assert r2 == recs, f"{mode}: records differ"
        for k in range(4):
            assert t2[k].tobytes() == tracks[k].tobytes(), f"{mode}: tracks of frame {k} differ"
        assert s2.tobytes() == signs.tobytes() and d2 == dropped, f"{mode}: signs differ"
        assert np.array_equal(c2, crops), f"{mode}: best crops differ"
