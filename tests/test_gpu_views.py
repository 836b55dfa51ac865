"""GPU tests of scaled views (lp_run_views, lp_run_views_device, the window gather through lp_test_view_windows) against NumPy,
the existing paths (lp_run_batch, lp_run_tiled) and the CPU oracle (tests/views_ref.py).  Models are seeded synthetic files
for det_input 320."""
import numpy as np
import pytest
import torch

import tiling_ref as T
import views_ref as V
from test_gpu_rect import tiled_rows_fit

pytestmark = pytest.mark.gpu

S = 320
H, W = 704, 896
CONF, IOU, MIN_AREA = 0.25, 0.45, 50
# the views of the end-to-end test: the whole frame, a half-scale window (bars top and bottom), a 1.6x up-scaled window
# (odd origin) and a native one
E2E_VIEWS = ["full", (100, 40, 640, 600), (301, 201, 200, 200), (500, 350, 320, 320)]
E2E_FRAME = 1
# what the fp32 oracle (CpuViewsPipeline.run_views on that frame with E2E_VIEWS at conf 0.25, iou 0.45, min_area 50) keeps after
# the frame NMS, computed on the CPU before the first GPU run
E2E_ORACLE_KEPT = 20


def _frames():
    from litepi import synth
    return [np.ascontiguousarray(f[:H, :W]) for f in synth.config4_images(2, seed=5, size=960, grain=8)]


def _calibrate_on_views(param, binf, views, lo, hi):
    """tests/test_gpu_tiling.py's procedure on S x S views given as pixels: shift the class biases so that between lo and hi
    candidates per view pass conf 0.25, with the threshold in the widest gap between two neighbouring scores of that range"""
    from litepi import ncnn_export
    from oracle import ncnn_ref, postprocess_ref as P
    layers = ncnn_ref.load_model(param, binf)
    with torch.no_grad():
        x = np.concatenate([P.preprocess(v, S)[0] for v in views])
        out = ncnn_ref.run_graph(layers, torch.from_numpy(x))["out0"].numpy()
    s = np.sort(out[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    ks = np.arange(lo * len(views), hi * len(views))
    k = int(ks[np.argmax(np.log(s[ks - 1] / (1 - s[ks - 1])) - np.log(s[ks] / (1 - s[ks])))])
    logit = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(param, binf, float(np.log(0.25 / 0.75) - logit))


def make_models(d):
    """the models of this file in directory d (also used to compute E2E_ORACLE_KEPT on the CPU)"""
    from litepi import ncnn_export
    from oracle import shufflenet_ref
    p, b = str(d / "m.param"), str(d / "m.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0, size=S)
    frames = _frames()
    _calibrate_on_views(p, b, [v for v, _, _ in V.make_views(frames[E2E_FRAME], S, E2E_VIEWS)], 4, 8)
    sd = shufflenet_ref.seeded_state_dict(91)
    cls_path = str(d / "cls.pth")
    torch.save(sd, cls_path)
    return dict(param=p, bin=b, cls=cls_path, sd=sd, frames=frames)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return make_models(tmp_path_factory.mktemp("views"))


def _engine(models, prec, max_batch, classifier=True):
    from litepi import Engine
    from litepi.backend import random_shufflenet_state
    e = Engine(precision=prec, max_batch=max_batch, max_det=300, num_classes=91, det_input=S)
    e.load_detector(models["param"], models["bin"])
    if classifier:
        e.load_classifier(random_shufflenet_state(91, seed=3))
    return e


# ---------------------------------------------------------------------------- 1. the gather against NumPy
# (x, y, w, h) windows per frame; det_input 64 is the smallest the library takes (one column tile), 320 has three
GATHER = {
    (150, 210): [(0, 0, 210, 150), "full", (1, 1, 96, 96), (169, 110, 40, 40), (73, 31, 64, 64), (5, 0, 16, 16), (0, 3, 210, 30),
                 (171, 0, 25, 150)],
    (333, 517): [(101, 57, 96, 96),                     # 1.5x down (at 64), odd x
                 (33, 20, 40, 40), (7, 9, 16, 16),      # 1.6x and 4x up
                 (211, 130, 64, 64), (453, 269, 64, 64), (0, 0, 64, 64), (13, 5, 320, 320),   # w = h = S: the copy branch
                 (0, 0, 517, 100), (400, 3, 50, 330),   # wide and tall: bars top / bottom and left / right
                 (437, 243, 80, 90),                    # ends on the frame's last pixel
                 (0, 0, 517, 333), "full"],
    (70, 720): [(0, 0, 720, 70),                        # 11.25x down at 64: the source span exceeds the LDS rows -> per-pixel kernel
                (5, 3, 64, 64), (0, 0, 96, 64), (700, 50, 20, 20), (1, 1, 40, 40), "full"],
    (60, 1400): [(0, 0, 1400, 60),                      # 4.4x down at 320 (only): staged, three column tiles, so the span's first byte
                 (3, 1, 1290, 58), "full"],             # lies far beyond the LDS shift; the second window's origin is odd
}
GATHER_CASES = [(shape, s) for s in (64, 320) for shape in GATHER if not (shape == (60, 1400) and s == 64)]


@pytest.fixture(scope="module")
def gather_engines():
    from litepi import Engine
    es = {s: Engine(precision="fp32", max_batch=16, max_det=8, num_classes=4, det_input=s) for s in (64, 320)}
    yield es
    for e in es.values():
        e.close()


@pytest.mark.parametrize("shape,s", GATHER_CASES, ids=[f"shape{list(GATHER).index(shape)}-{s}" for shape, s in GATHER_CASES])
def test_window_gather_bytes_equal_numpy(gather_engines, shape, s):
    eng = gather_engines[s]
    rng = np.random.default_rng(shape[0] * 7 + s)
    img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    views = GATHER[shape]
    exp = np.stack([V.make_view(img, s, v)[0] for v in views])
    scales = [V.window(v, *shape)[2] / V.view_geometry(s, *shape, v)["new_w"] for v in views]
    if s == 64:
        assert max(scales) > 10 or shape != (70, 720), "the per-pixel fallback is not reached"
    if shape == (60, 1400):   # the launcher's row rule, computed on the CPU: every window is staged, none falls back
        assert min(scales) > 4 and all(tiled_rows_fit(V.view_geometry(s, *shape, v)["new_w"], V.window(v, *shape)[2]) for v in views)
    lists = [views] if max(scales) <= 10 else [views, [v for v, sc in zip(views, scales) if sc <= 10]]   # with / without the fallback
    for lst in lists:
        want = exp[[views.index(v) for v in lst]]
        for off in (0, 1, 7, 48):
            got = eng.test_view_windows(img, lst, byte_offset=off)
            for k, v in enumerate(lst):
                assert np.array_equal(got[k], want[k]), (f"{shape} S {s} offset {off} view {v}: {int((got[k] != want[k]).sum())} bytes differ, "
                                                         f"first at {np.argwhere(got[k] != want[k])[0].tolist()}")
    for k, v in enumerate(views):   # and the letterbox of the sub-image copied out contiguously
        x, y, w, h = V.window(v, *shape)
        lb, r, pad = eng.test_letterbox(np.ascontiguousarray(img[y:y + h, x:x + w]))
        assert np.array_equal(lb, exp[k]), f"{shape} S {s} view {v}: lp_test_letterbox of the crop differs"
        g = eng.view_geometry(shape[0], shape[1], v)
        assert np.float32(r) == g["ratio"]
        if x == 0 and y == 0:
            assert (np.float32(pad[0]), np.float32(pad[1])) == (g["pad_w"], g["pad_h"])


# ---------------------------------------------------------------------------- 2. equalities with the existing paths
def _same_host(got, ref, avg, ref_avg, B, tag):
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), f"{tag}: counts {got[1]} / {got[2]} vs {ref[1]} / {ref[2]}"
    assert np.array_equal(avg.view(np.uint32), ref_avg.view(np.uint32)), f"{tag}: det_conf_avg"
    for i in range(B):
        n = int(ref[1][i])
        assert got[0][i, :n].tobytes() == ref[0][i, :n].tobytes(), f"{tag} frame {i}: records differ"


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_views_equal_run_batch_and_run_tiled(models, prec):
    frames = models["frames"]
    B = len(frames)
    grid = T.tile_grid(S, H, W, 64, True)
    assert len(grid) == 13
    e = _engine(models, prec, B * len(grid))
    try:
        assert e.tile_grid(H, W, 64, True) == grid == e.view_grid(H, W, S, 64, True)
        ref = e.run_batch(frames, CONF, IOU, MIN_AREA)
        ref_avg = e.last_det_conf_avg.copy()
        assert int(ref[1].sum()) >= 1, "run_batch found nothing: the comparison is empty"
        for call in range(3):   # eager, captured, replayed
            got = e.run_views(frames, ["full"], CONF, IOU, MIN_AREA)
            _same_host(got, ref, e.last_det_conf_avg, ref_avg, B, f"{prec} full call {call}")
        ref = e.run_tiled(frames, CONF, IOU, MIN_AREA, overlap=64, full_frame=True)
        ref_avg = e.last_det_conf_avg.copy()
        assert int(ref[1].sum()) >= 1, "run_tiled found nothing: the comparison is empty"
        for call in range(3):
            got = e.run_views(frames, grid, CONF, IOU, MIN_AREA)
            _same_host(got, ref, e.last_det_conf_avg, ref_avg, B, f"{prec} tile grid call {call}")
    finally:
        e.close()


# ---------------------------------------------------------------------------- 3. fp32 end to end against the oracle
def test_views_fp32_end_to_end_vs_oracle(models):
    """Tolerances of test_tiled_fp32_end_to_end_vs_oracle: score 1e-3, box 1 px, classes and num_det equal."""
    from litepi import HybridPipeline
    from oracle import ncnn_ref, shufflenet_ref
    frame = models["frames"][E2E_FRAME]
    cpu = V.CpuViewsPipeline(ncnn_ref.load_model(models["param"], models["bin"]), shufflenet_ref.build(91, models["sd"]), input_size=S)
    exp, exp_num = cpu.run_views(frame, E2E_VIEWS, CONF, IOU, MIN_AREA)
    print(f"oracle: {exp_num} kept after the frame NMS, {len(exp)} after the area filter")
    assert exp_num == E2E_ORACLE_KEPT, f"the oracle keeps {exp_num}, the literal says {E2E_ORACLE_KEPT}"
    assert E2E_ORACLE_KEPT >= 4, "calibration produced too few detections for a meaningful test"
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, det_input_size=S,
                          precision="fp32", max_batch=4, max_det=300, views=E2E_VIEWS)
    try:
        res, met = pipe.run_batch([frame], CONF, IOU, MIN_AREA)[0]
    finally:
        pipe.engine.close()
    print(f"device: num_det {met.num_detections}, {len(res)} results")
    assert met.num_detections == exp_num, f"num_det {met.num_detections} vs oracle {exp_num}"
    assert len(res) == len(exp), f"{len(res)} results vs oracle {len(exp)}"
    for r, x in zip(res, exp):
        assert abs(r["det_conf"] - x["det_conf"]) <= 1e-3
        assert np.abs(np.array(r["bbox"]) - np.array(x["bbox"])).max() <= 1
        assert r["det_class"] == x["det_class"] and r["cls_class"] == x["cls_class"]


# ---------------------------------------------------------------------------- 4. device path
@pytest.mark.parametrize("fmt", ["bgr", "nv12"])
def test_views_device_path_equals_host_path(models, fmt):
    import pixfmt_ref as R
    from litepi._ffi import DET_DTYPE
    lists = {"A": E2E_VIEWS, "B": V.view_grid(640, H, W, 128, True)}
    assert len(lists["B"]) == 5
    frames = [models["frames"][0], models["frames"][1]]
    flipped = [np.ascontiguousarray(f[:, ::-1]) for f in frames]
    if fmt == "nv12":
        frames, flipped = [R.bgr_to_nv12(f) for f in frames], [R.bgr_to_nv12(f) for f in flipped]
    B = 2
    e = _engine(models, "fp16", 16)
    try:
        e.set_input_format(fmt)
        refs = {}
        for name, views in lists.items():
            for which, fs in (("plain", frames), ("flipped", flipped)):
                d, c, nd, _ = e.run_views(fs, views, CONF, IOU, MIN_AREA)
                refs[name, which] = (d.copy(), c.copy(), nd.copy(), e.last_det_conf_avg.copy())
        assert sum(int(r[2].sum()) for r in refs.values()) >= 4 and all(int(r[2].sum()) >= 1 for r in refs.values())
        bufs = {"plain": torch.from_numpy(np.stack(frames)).cuda(), "flipped": torch.from_numpy(np.stack(flipped)).cuda()}
        dd = torch.zeros(B * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for call, name in enumerate("AAABBAB"):   # eager, capturing, replayed; two input buffers and two view lists alternate
            which = ("plain", "flipped")[call % 2]
            e.run_views_device(bufs[which].data_ptr(), B, H, W, lists[name], CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            dets_ref, counts_ref, num_ref, avg_ref = refs[name, which]
            cnt = dc.cpu().numpy()
            tag = f"{fmt} call {call} list {name} {which}"
            assert np.array_equal(cnt[:B], counts_ref) and np.array_equal(cnt[B:2 * B], num_ref), tag
            assert np.array_equal(cnt[2 * B:].view(np.uint32), avg_ref.view(np.uint32)), tag
            recs = dd.cpu().numpy().view(DET_DTYPE).reshape(B, -1)
            for i in range(B):
                assert recs[i, :counts_ref[i]].tobytes() == dets_ref[i, :counts_ref[i]].tobytes(), f"{tag} frame {i}"
    finally:
        e.close()


# ---------------------------------------------------------------------------- 5. errors
def test_views_errors_leave_the_handle_usable(models):
    from litepi._ffi import LP_ERR_ARG, LitepiError
    frames = models["frames"]
    e = _engine(models, "fp16", 4)
    try:
        good = ["full", (100, 40, 640, 600)]
        ref = e.run_views(frames, good, CONF, IOU, MIN_AREA)
        dd = torch.zeros(2 * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(6, dtype=torch.int32, device="cuda")
        dev = torch.from_numpy(np.stack(frames)).cuda()
        torch.cuda.synchronize()
        bad_lists = {"a window passing the frame edge": ["full", (600, 40, 297, 100)],
                     "a window passing the lower edge": [(0, 700, 100, 16)],
                     "w = 15": ["full", (10, 10, 15, 100)],
                     "n_views = 0": [],
                     "B x n_views > max_batch": ["full", (0, 0, 320, 320), (100, 40, 640, 600)]}
        for what, bad in bad_lists.items():
            with pytest.raises(LitepiError) as ex:
                e.run_views(frames, bad, CONF, IOU, MIN_AREA)
            assert ex.value.code == LP_ERR_ARG, what
            got = e.run_views(frames, good, CONF, IOU, MIN_AREA)   # the handle is still usable, with the same result
            _same_host(got, ref, e.last_det_conf_avg, e.last_det_conf_avg, 2, f"after {what}")
            with pytest.raises(LitepiError) as ex:
                e.run_views_device(dev.data_ptr(), 2, H, W, bad, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
            assert ex.value.code == LP_ERR_ARG, what + " (device)"
            e.run_views_device(dev.data_ptr(), 2, H, W, good, CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
            e.synchronize()
            assert np.array_equal(dc.cpu().numpy()[:2], ref[1]), f"device call after {what}"
        # a window that fits the first frame but not a smaller second one: every frame of the call counts
        with pytest.raises(LitepiError) as ex:
            e.run_views([frames[0], np.ascontiguousarray(frames[1][:600])], good, CONF, IOU, MIN_AREA)
        assert ex.value.code == LP_ERR_ARG
        e.run_views(frames, good, CONF, IOU, MIN_AREA)
    finally:
        e.close()


# ---------------------------------------------------------------------------- 6. tracker and inventory
def test_views_pipeline_tracks_and_collects_signs(models):
    from litepi import HybridPipeline
    rng = np.random.default_rng(3)
    patch = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    seq = []
    for k in range(6):
        f = models["frames"][0].copy()
        f[300:396, 400 + 4 * k:496 + 4 * k] = patch
        seq.append(f)
    views = ["full", (100, 40, 640, 600), (301, 201, 320, 320)]
    tcfg = dict(n_streams=1, max_tracks=256, max_age=1, min_hits=2, iou_match=0.3)
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, det_input_size=S,
                          precision="fp16", max_batch=4, max_det=300, views=views, track=True, track_config=tcfg, inventory=True)
    e = _engine(models, "fp16", 4, classifier=False)
    try:
        e.load_classifier(models["sd"])
        e.tracker_create(**tcfg)
        n_tracked = 0
        for k, f in enumerate(seq):
            res, _ = pipe.run_batch([f], CONF, IOU, MIN_AREA)[0]
            d, c, _, _ = e.run_views([f], views, CONF, IOU, MIN_AREA)
            tr = e.track(d, np.asarray(c, dtype=np.int32))
            n = int(c[0])
            assert len(res) == n, f"frame {k}: {len(res)} results vs {n} records"
            got = [(r["track_id"], r["track_hits"], r["track_age"], r["track_cls"], r["track_confirmed"]) for r in res]
            want = [(int(t["track_id"]), int(t["hits"]), int(t["age"]), int(t["voted_class"]), bool(t["flags"] & 1)) for t in tr[0, :n]]
            assert got == want, f"frame {k}: tracker records differ"
            assert [r["det_conf"] for r in res] == [float(x) for x in d[0, :n]["det_conf"]]
            n_tracked += sum(1 for t in want if t[0] > 0 and t[1] >= 2)
        assert n_tracked >= 1, "no detection was tracked over two frames: the comparison is empty"
        signs = pipe.drain_signs(flush=True)
        assert signs and any(s["crop"] is not None for s in signs), "no sign with a crop came out"
        assert all(s["crop"] is None or s["crop"].shape == (64, 64, 3) for s in signs)
    finally:
        pipe.close()
        e.close()


# ---------------------------------------------------------------------------- 7. the pipeline's view_tile mode, chunked over max_batch
def test_views_pipeline_view_tile_chunks_over_max_batch(models):
    """HybridPipeline(view_tile=...) takes every frame's window grid from its size and splits a batch into lp_run_views calls
    of consecutive frames that share a list and fit max_batch: four frames of two sizes (7, 7, 5 and 5 views) on a 12-view
    handle are three calls, and every frame's result equals lp_run_views on that frame alone with its own grid."""
    from litepi import HybridPipeline
    f0, f1 = models["frames"]
    frames = [f0, f1, np.ascontiguousarray(f0[:600, :800]), np.ascontiguousarray(f1[:600, :800])]
    grids = [V.view_grid(480, f.shape[0], f.shape[1], 96, True) for f in frames]
    assert [len(g) for g in grids] == [7, 7, 5, 5]
    pipe = HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, det_input_size=S,
                          precision="fp16", max_batch=12, max_det=300, view_tile=480, view_overlap=96)
    try:
        outs = pipe.run_batch(frames, CONF, IOU, MIN_AREA)
        total = 0
        for k, (f, g) in enumerate(zip(frames, grids)):
            d, c, nd, _ = pipe.engine.run_views([f], g, CONF, IOU, MIN_AREA)
            res, met = outs[k]
            n = int(c[0])
            assert met.num_detections == int(nd[0]) and len(res) == n, f"frame {k}"
            assert [(r["det_conf"], r["cls_class"], r["cls_conf"]) for r in res] == \
                   [(float(x["det_conf"]), int(x["cls_class"]), float(x["cls_conf"])) for x in d[0, :n]], f"frame {k}"
            total += n
        assert total >= 4, "too few detections for a meaningful comparison"
        with pytest.raises(ValueError):
            HybridPipeline(models["param"], models["bin"], models["cls"], "shufflenetv2", num_classes=91, det_input_size=S,
                           view_tile=480, tile_overlap=64)
    finally:
        pipe.close()
