"""The classifier's GPU paths against a float64 oracle, in log p (``-m gpu``).

Metric: element-wise |log p_gpu - log p_ref| over all ROIs and classes of the 64-ROI pool (tests/classifier_pool.py), with
p_ref the float64 module (oracle/shufflenet_ref.py).  Bounds:
  fp16 paths (A, B, C): max <= 2 x and mean <= 1.5 x the error of that path's fp16-storage emulation
      (shufflenet_ref.RECIPES: rounding where the path's code stores fp16), computed here on the same ROIs.  The kernels round
      the same tensors; what differs is fp32 accumulation order, far below fp16 rounding.
  fp32 paths (D, E, other architectures): max <= 10 x the gap between the float32 torch module and the float64 one on the
      same ROIs (both sum in fp32 in different orders; the GPU also has its own expf and division).
  argmax: the reference argmax, or a class whose reference log p is within 2 x bound of the reference maximum.

Paths, each proved by the kernel names the profiler saw on its first call:
  A fp16 default (cls_front_f16 + cls_back_f16)       B fp16 LITEPI_CLS_LAYERWISE=1 (shuffle_stage_fused_f16,
  C fp16 conv_impl=1 (conv_naive_f16)                   cls_head_fused_f16; the switch is read once per load_classifier)
  D fp32 conv_impl=0 (conv1x1_mfma_f32)               E fp32 conv_impl=1 (conv_naive_f32)

Within one handle no kernel reduces across ROIs, so a ROI's probabilities and id must be bit-equal whatever batch it sits
in: the ROI-count cases (grid-stride passes past 1024 ROIs included) and the pipeline's scatter into detection records are
checked that way."""
import functools

import numpy as np
import pytest
import torch

import classifier_pool as CP
from oracle import shufflenet_ref as S

pytestmark = pytest.mark.gpu

# path: (precision, conv_impl, emulation recipe (None: fp32), kernel names that must have run)
PATHS = {
    "A": ("fp16", 0, "fused", {"cls_front_f16", "cls_back_f16"}),
    "B": ("fp16", 0, "layerwise", {"shuffle_stage_fused_f16", "cls_head_fused_f16"}),
    "C": ("fp16", 1, "naive", {"conv_naive_f16"}),
    "D": ("fp32", 0, None, {"conv1x1_mfma_f32"}),
    "E": ("fp32", 1, None, {"conv_naive_f32"}),
}
POOL_COUNTS = [("A", n) for n in (2, 58, 64, 65, 91, 129, 560)] + [(p, n) for p in "CDE" for n in (2, 91, 600)]
COUNT_CASES = [("A",) + c for c in CP.A_CASES] + [(p,) + c for p in "CDE" for c in CP.OTHER_CASES]


@functools.lru_cache(maxsize=None)
def _pool():
    return CP.pool()


@functools.lru_cache(maxsize=None)
def _x():
    return S.input_batch(_pool())


@functools.lru_cache(maxsize=None)
def _sd(nc):
    return S.seeded_state_dict(nc)


@functools.lru_cache(maxsize=None)
def _ref(nc):
    return S.logp_module(S.build(nc, _sd(nc)), _x())


@functools.lru_cache(maxsize=None)
def _bound(nc, path):
    """The path's bound on the pool at nc classes (see the module docstring)."""
    ref = _ref(nc)
    recipe = PATHS[path][2]
    if recipe is None:
        gap = np.abs(S.logp_module(S.build(nc, _sd(nc)), _x(), torch.float32) - ref).max()
        return dict(fp16=False, oracle_max=gap, max=10 * gap)
    e = np.abs(S.folded_logp(_sd(nc), _pool(), recipe) - ref)
    return dict(fp16=True, oracle_max=e.max(), oracle_mean=e.mean(), max=2 * e.max(), mean=1.5 * e.mean())


def _np_sd(sd):
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}


def _job(path, nc, cap, calls, sd=None, arch="shufflenetv2"):
    prec, impl = PATHS[path][:2]
    return dict(prec=prec, impl=impl, nc=nc, cap=cap, calls=[np.asarray(c, np.int64) for c in calls],
                sd=_np_sd(_sd(nc) if sd is None else sd), arch=arch, load_env=LAYERWISE_ENV if path == "B" else {})


def _count_calls(cap, R):
    """pool (chunks of cap), then the R-slot batch, then slots 0, R/2 and R-1 each alone"""
    idx = CP.draw(cap, R)
    ks = sorted({0, R // 2, R - 1})
    return [np.arange(64), idx] + [idx[k:k + 1] for k in ks], idx, ks


LAYERWISE_ENV = {"LITEPI_CLS_LAYERWISE": "1"}   # set around load_classifier only: Classifier::load reads it once per load


def _run(path, job, monkeypatch=None):
    assert bool(job["load_env"]) == (path == "B")
    return CP.run_job(job, _pool(), monkeypatch)


def _check_names(path, res):
    want = PATHS[path][3]
    assert not res["error"], res["error"]
    assert want <= set(res["names"]), f"path {path}: expected kernels {sorted(want)}, profiler saw {res['names']}"
    if path in "BCDE":
        assert not any(n.startswith("cls_front") or n.startswith("cls_back") for n in res["names"]), res["names"]


FP32_TINY = float(np.finfo(np.float32).tiny)
LOG_LIVE = np.log(FP32_TINY) + 1.0   # below it a reference probability is within e of fp32's smallest normal number


def _check_vs_ref(label, probs, ids, ref, b):
    """log p bound and argmax rule against the float64 reference ref [N, classes].  The probabilities come back as fp32: where
    the reference's is too small for a normal fp32 number (log p < log(FLT_MIN) + 1: subnormal or zero, no relative
    precision left) the GPU's must be at most FLT_MIN and is left out of the log p metric.  (Only EfficientNet-B0's seeded
    weights reach there, down to log p = -114; the ShuffleNetV2 pool stays above -15.)"""
    N, nc = ref.shape
    assert probs.shape == (N, nc) and ids.shape == (N,)
    assert ((ids >= 0) & (ids < nc)).all(), f"{label}: ids out of range {ids}"
    live = ref > LOG_LIVE
    assert (probs[~live] <= FP32_TINY).all(), f"{label}: probabilities the reference puts below fp32's normal range"
    with np.errstate(divide="ignore"):
        err = np.where(live, np.abs(np.log(probs.astype(np.float64)) - ref), 0.0)
    top = ref.max(axis=1)
    ok_id = (ids == ref.argmax(axis=1)) | (ref[np.arange(N), ids] >= top - 2 * b["max"])
    if b["fp16"]:
        print(f"CLS {label}: log p err max {err.max():.3e} mean {err.mean():.3e} | emulation max {b['oracle_max']:.3e} "
              f"mean {b['oracle_mean']:.3e} | bound max {b['max']:.3e} mean {b['mean']:.3e} | argmax = ref {np.mean(ids == ref.argmax(1)):.3f}")
    else:
        print(f"CLS {label}: log p err max {err.max():.3e} | fp32 oracle gap {b['oracle_max']:.3e} | bound {b['max']:.3e} | "
              f"argmax = ref {np.mean(ids == ref.argmax(1)):.3f}")
    assert np.isfinite(err).all(), f"{label}: zero / non-finite probabilities"
    assert err.max() <= b["max"], f"{label}: max {err.max():.3e} > {b['max']:.3e}"
    if b["fp16"]:
        assert err.mean() <= b["mean"], f"{label}: mean {err.mean():.3e} > {b['mean']:.3e}"
    assert ok_id.all(), f"{label}: arg-max outside the bound for ROIs {np.flatnonzero(~ok_id)}"


def _bits_equal(a, b):
    return np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)


def _check_counts(label, res, cap, R, ref, b):
    """pool baseline under the bound; every slot of the R batch and every single-ROI call bit-equal to the baseline"""
    calls, idx, ks = _count_calls(cap, R)
    assert not res["error"], res["error"]
    assert len(res["probs"]) == len(calls)
    base_ids, base_p = res["ids"][0], res["probs"][0]
    _check_vs_ref(f"{label} cap {cap} pool", base_p, base_ids, ref, b)
    ids, probs = res["ids"][1], res["probs"][1]
    assert probs.shape == (R, ref.shape[1])
    same = _bits_equal(probs, base_p[idx]).all(axis=1) & (ids == base_ids[idx])
    print(f"CLS {label} ({cap}, {R}): {int(same.sum())} of {R} slots bit-equal to the handle's baseline")
    assert same.all(), f"{label} ({cap}, {R}): {int((~same).sum())} slots differ, first {np.flatnonzero(~same)[:8].tolist()}"
    for n, k in enumerate(ks):
        one_ids, one_p = res["ids"][2 + n], res["probs"][2 + n]
        assert one_ids[0] == ids[k] and _bits_equal(one_p[0], probs[k]).all(), f"{label} ({cap}, {R}): slot {k} alone differs"


def _check_ties(label, res, pair):
    lo, hi = pair
    assert not res["error"], res["error"]
    ids, probs = res["ids"][0], res["probs"][0]
    print(f"CLS {label} tie {pair}: ids {np.unique(ids).tolist()}, columns bit-equal {bool(_bits_equal(probs[:, lo], probs[:, hi]).all())}")
    assert _bits_equal(probs[:, lo], probs[:, hi]).all(), f"{label}: the tied columns differ"
    assert (ids == lo).all(), f"{label}: ids {np.unique(ids).tolist()} instead of the lower index {lo}"


# ------------------------------------------------------------------------------------------------------ paths A, C, D, E
@pytest.mark.parametrize("path,nc", POOL_COUNTS, ids=[f"{p}-{n}" for p, n in POOL_COUNTS])
def test_pool_vs_float64(path, nc):
    res = _run(path, _job(path, nc, 64, [np.arange(64)]))
    _check_names(path, res)
    _check_vs_ref(f"path {path} {nc} classes", res["probs"][0], res["ids"][0], _ref(nc), _bound(nc, path))


@pytest.mark.parametrize("path", ["A", "D"])
def test_one_class(path):
    res = _run(path, _job(path, 1, 64, [np.arange(64)]))
    _check_names(path, res)
    ids, probs = res["ids"][0], res["probs"][0]
    assert probs.shape == (64, 1) and (probs == 1.0).all() and (ids == 0).all()


def test_too_many_classes_refused_fused():
    """cls_back keeps 4 ROIs' logits in LDS: nc_p <= 560.  561 classes must be refused, never answered."""
    res = _run("A", _job("A", 561, 64, [np.arange(64)]))
    print(f"CLS path A 561 classes: {res['error']!r}")
    assert res["error"] and not res["probs"]


@pytest.mark.parametrize("pair", CP.TIE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
@pytest.mark.parametrize("path", ["A", "D"])
def test_argmax_ties(path, pair):
    """Two identical fc rows and biases, raised to the top two of every ROI: the id is the lower index (np.argmax), the two
    columns' probabilities are bit-equal."""
    tsd = CP.tie_state_dict(_sd(91), pair, _ref(91))
    res = _run(path, _job(path, 91, 64, [np.arange(64)], sd=tsd))
    _check_names(path, res)
    _check_ties(f"path {path}", res, pair)


@pytest.mark.parametrize("path,cap,R", COUNT_CASES, ids=[f"{p}-{c}-{r}" for p, c, r in COUNT_CASES])
def test_roi_count_invariance(path, cap, R):
    """One handle per capacity (max_batch 1, max_det = max_rois = cap): the pool under the bound, then R slots drawn from it
    (cls_back's second grid pass starts past 1024 ROIs) bit-equal to that baseline, and slots 0, R/2, R-1 alone."""
    calls, _, _ = _count_calls(cap, R)
    res = _run(path, _job(path, 91, cap, calls))
    _check_names(path, res)
    _check_counts(f"path {path}", res, cap, R, _ref(91), _bound(91, path))


# ---------------------------------------------------------------------------------------------------------------- path B
B_JOBS = {
    "pool-91": (91, 64, None, [np.arange(64)]),
    "pool-256": (256, 64, None, [np.arange(64)]),
    "refuse-257": (257, 64, None, [np.arange(64)]),
    **{f"tie-{p[0]}-{p[1]}": (91, 64, p, [np.arange(64)]) for p in CP.TIE_PAIRS},
    **{f"count-{c}-{r}": (91, c, None, _count_calls(c, r)[0]) for c, r in CP.OTHER_CASES},
}


def _run_b(name, monkeypatch):
    nc, cap, pair, calls = B_JOBS[name]
    sd = CP.tie_state_dict(_sd(nc), pair, _ref(nc)) if pair else None
    return _run("B", _job("B", nc, cap, calls, sd=sd), monkeypatch)


@pytest.mark.parametrize("nc", [91, 256])
def test_layerwise_pool_vs_float64(monkeypatch, nc):
    res = _run_b(f"pool-{nc}", monkeypatch)
    _check_names("B", res)
    _check_vs_ref(f"path B {nc} classes", res["probs"][0], res["ids"][0], _ref(nc), _bound(nc, "B"))


def test_layerwise_too_many_classes_refused(monkeypatch):
    """cls_head_fused accepts nc_p <= 256: 257 classes must be refused, never answered."""
    res = _run_b("refuse-257", monkeypatch)
    print(f"CLS path B 257 classes: {res['error']!r}")
    assert res["error"] and not res["probs"]


@pytest.mark.parametrize("pair", CP.TIE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_layerwise_argmax_ties(monkeypatch, pair):
    res = _run_b(f"tie-{pair[0]}-{pair[1]}", monkeypatch)
    _check_names("B", res)
    _check_ties("path B", res, pair)


@pytest.mark.parametrize("cap,R", CP.OTHER_CASES, ids=[f"{c}-{r}" for c, r in CP.OTHER_CASES])
def test_layerwise_roi_count_invariance(monkeypatch, cap, R):
    res = _run_b(f"count-{cap}-{R}", monkeypatch)
    _check_names("B", res)
    _check_counts("path B", res, cap, R, _ref(91), _bound(91, "B"))


def test_plan_is_chosen_per_load(monkeypatch):
    """Two handles in one process (capacity 64, 91 classes), the first loaded with LITEPI_CLS_LAYERWISE set and the second
    without, called alternately twice each on the pool: each handle's profiler names are its own plan's (PATHS) on every call, and
    its second result is bit-equal to its first."""
    from litepi import Engine
    sd, rois = _np_sd(_sd(91)), _pool()
    engines, got = {}, {"B": [], "A": []}
    try:
        for path in "BA":
            engines[path] = Engine(precision="fp16", max_batch=1, max_det=64, num_classes=91, max_rois=64, conv_impl=0, cls_arch="shufflenetv2")
            with monkeypatch.context() as m:
                m.delenv("LITEPI_CLS_LAYERWISE", raising=False)
                if path == "B":
                    m.setenv("LITEPI_CLS_LAYERWISE", "1")
                engines[path].load_classifier(sd)
        for _ in range(2):
            for path, e in engines.items():
                e.profile_next(True)
                ids, probs = e.classify(rois)
                _check_names(path, dict(error="", names=sorted({k["name"] for k in e.profile_read()})))
                got[path].append((ids, probs))
    finally:
        for e in engines.values():
            e.close()
    for path, ((ids0, p0), (ids1, p1)) in got.items():
        assert p0.shape == (64, 91) and (ids0 == ids1).all() and _bits_equal(p0, p1).all(), f"path {path}: the second call differs from the first"


# ------------------------------------------------------------------------------------- routing through the pipeline
@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_pipeline_routes_results_to_their_records(tmp_path, prec):
    """One run_batch call of 8 frames classifies >= 1100 ROIs (cls_back's grid-stride pass included); on eager, captured and
    replayed calls every record's (cls_class, cls_conf) is bit-equal to pipe.engine.classify of that record's own crop on the
    same handle (rectangles from the oracle's postprocess + roi_rects on the device's own out0)."""
    from litepi import HybridPipeline, ncnn_export
    from oracle import postprocess_ref as P
    from test_gpu_parity import _calibrate
    p, b = str(tmp_path / "m.param"), str(tmp_path / "m.bin")
    ncnn_export.export_detector(p, b, "v1", seed=77, cls_bias=0.0)
    imgs = np.random.default_rng(2024).integers(0, 256, (8, 640, 640, 3), dtype=np.uint8)
    _calibrate(p, b, imgs, 300)
    cls_path = str(tmp_path / "cls.pth")
    torch.save(_sd(91), cls_path)
    conf, iou, min_area = 0.25, 0.45, 50
    pipe = HybridPipeline(p, b, cls_path, "shufflenetv2", num_classes=91, precision=prec, max_batch=8, max_det=300)
    try:
        got0 = pipe.engine.detect_raw(imgs)
        crops, where = [], []
        for i in range(8):
            eb, es, _ = P.postprocess(got0[i], (640, 640), 1.0, (0.0, 0.0), conf, iou)
            top = np.sort(np.argsort(-es, kind="stable")[:300])
            rects, valid = P.roi_rects(eb[top], 640, 640, min_area)
            crops += [imgs[i][y1:y2, x1:x2] for x1, y1, x2, y2 in rects]
            where += [(i, n, tuple(eb[top][k].astype(int))) for n, k in enumerate(valid)]
        assert len(crops) >= 1100, f"calibration gave {len(crops)} ROIs for one call, need >= 1100"
        ids, probs = pipe.engine.classify(crops)
        for call in ("eager", "capture", "replay"):
            outs = pipe.run_batch(list(imgs), conf, iou, min_area)
            n_res = [len(outs[i][0]) for i in range(8)]
            assert sum(n_res) == len(crops), f"{call}: {n_res} records vs {len(crops)} oracle ROIs"
            bad = 0
            for k, (i, n, box) in enumerate(where):
                r = outs[i][0][n]
                assert r["bbox"] == box, f"{call}: image {i} record {n}: bbox {r['bbox']} vs {box}"
                ok = r["cls_class"] == int(ids[k]) and np.float32(r["cls_conf"]).view(np.uint32) == probs[k, ids[k]].view(np.uint32)
                bad += 0 if ok else 1
            print(f"CLS pipeline {prec} {call}: {len(crops)} ROIs in one call, {bad} records differ from classify")
            assert bad == 0, f"{call}: {bad} of {len(crops)} records carry another ROI's (class, confidence)"
    finally:
        pipe.close()


# --------------------------------------------------------------------------------------- the other three architectures
def _arch(arch, nc=58):
    if arch == "resnet18":
        from oracle import resnet_ref as R
        sd = R.seeded_state_dict(nc)
        return sd, R.build(nc, sd)
    from oracle import mbnet_ref as M
    sd = M.seeded_state_dict(arch, nc)
    return sd, M.build(arch, nc, sd)


@functools.lru_cache(maxsize=None)
def _arch_ref(arch):
    sd, model = _arch(arch)
    ref = S.logp_module(model, _x())
    gap = np.abs(S.logp_module(model, _x(), torch.float32) - ref).max()
    return sd, ref, dict(fp16=False, oracle_max=gap, max=10 * gap)


OTHER_ARCHS = ["resnet18", "mobilenetv2", "efficientnet"]


@pytest.mark.parametrize("arch", OTHER_ARCHS)
def test_other_arch_fp32_vs_float64(arch):
    sd, ref, b = _arch_ref(arch)
    res = CP.run_job(dict(prec="fp32", impl=0, nc=58, cap=64, calls=[np.arange(64)], sd=_np_sd(sd), arch=arch), _pool())
    assert not res["error"], res["error"]
    _check_vs_ref(f"{arch} fp32", res["probs"][0], res["ids"][0], ref, b)


@pytest.mark.parametrize("cout,use_res", [(40, False), (40, True), (88, False), (88, True)])
def test_conv1x1_fp16_channel_count_ending_inside_a_store_pair(cout, use_res):
    """The fp16 1x1 epilogue stores two channel quads at a time.  With 3 channel tiles per workgroup a lane's quads start at
    12g + 48ns, so a Cout of 40 or 88 (EfficientNet-B0's 40-channel projections) ends between the two quads of a pair; the
    store must then stop at Cout instead of writing the next pixel's first 4 channels (output pitch = Cout).  8 x 64 x 64
    pixels keep the 3-tile plan (>= 128 pixel blocks).  Bound as test_gpu_parity.py::test_conv_fp16: fp16-rounded inputs,
    one fp16 ulp of the output + slack."""
    import torch.nn.functional as F
    from litepi import Engine
    g = torch.Generator().manual_seed(cout + use_res)
    cin, N, H = 240, 8, 64
    x = torch.randn(N, cin, H, H, generator=g).half().float()
    w = (torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin) ** 0.5).half().float()
    b = torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(x.double(), w.double(), b.double())
    res = torch.randn(ref.shape, generator=g).half().float() if use_res else None
    if use_res:
        ref = ref + res.double()
    e = Engine(precision="fp16", max_batch=1, max_det=64, num_classes=91)
    try:
        y = e.test_conv(x.numpy(), w.numpy(), b.numpy(), stride=1, act=0, res=None if res is None else res.numpy())
    finally:
        e.close()
    err = np.abs(y - ref.numpy())
    tol = 2e-3 + 2e-3 * np.abs(ref.numpy())
    bad = err > tol
    print(f"CLS conv1x1 fp16 {cin}->{cout} res={use_res}: max err {err.max():.3e}, {int(bad.sum())} elements over the bound, "
          f"channels {sorted(set(np.nonzero(bad)[1].tolist()))[:8]}")
    assert not bad.any()


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
@pytest.mark.parametrize("arch", OTHER_ARCHS)
def test_other_arch_roi_count_invariance(arch, prec):
    """(1100, 1025) on one handle: every slot bit-equal to the handle's own pool baseline (fp16 keeps its probability bound
    in tests/test_gpu_parity.py; fp32 is also held to the log p bound here)."""
    cap, R = 1100, 1025
    sd, ref, b = _arch_ref(arch)
    calls, idx, ks = _count_calls(cap, R)
    res = CP.run_job(dict(prec=prec, impl=0, nc=58, cap=cap, calls=calls, sd=_np_sd(sd), arch=arch), _pool())
    assert not res["error"], res["error"]
    if prec == "fp32":
        _check_counts(f"{arch} fp32", res, cap, R, ref, b)
        return
    base_ids, base_p = res["ids"][0], res["probs"][0]
    ids, probs = res["ids"][1], res["probs"][1]
    same = _bits_equal(probs, base_p[idx]).all(axis=1) & (ids == base_ids[idx])
    print(f"CLS {arch} fp16 ({cap}, {R}): {int(same.sum())} of {R} slots bit-equal to the handle's baseline")
    assert same.all(), f"{arch} fp16: {int((~same).sum())} slots differ, first {np.flatnonzero(~same)[:8].tolist()}"
    for n, k in enumerate(ks):
        assert res["ids"][2 + n][0] == ids[k] and _bits_equal(res["probs"][2 + n][0], probs[k]).all(), f"{arch} fp16: slot {k} alone differs"
