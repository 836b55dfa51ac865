"""CPU tests of tests/head_ref.py, the float64 restatement of one level of the Detect head that test_gpu_head_float64.py holds
the fp16 head kernels against: the restatement computes what the oracle's graph computes, its error budget holds for a correct
fp16 implementation that is not the kernel, and the budget's caps catch the errors a tiled kernel makes.

Cases: the GPU module's models and images (the exporter's v1 and v2 at 320, batch 5, one class and at 352, batch 2, three classes),
the class bias calibrated to ~8 candidates per image -- here from the oracle's out0 -- so that scores spread over (0, 1).  Both modules
share models and images because the floor on max(e) is a property of those, not of any code under test: on another seeded v1 model
with two 320 x 320 images the score rows of P5 (200 anchors, all far below conf) measured max e = 8.9e-6, under the 1e-5 floor.

Measured here: float64 head against the fp32 oracle's out0 5.9e-5 ... 1.4e-4 (fp32 noise of the oracle; bound 1e-3 + 1e-3 |ref|); stand-in
kernel max d / max e <= 0.93, mean d / mean e <= 0.10 over every case, level and row group, fp16 logits included; every mutation
exceeds a cap at least 7.8 times over on every level it touches (the closest: dfl_w[15] = 14; a dropped halo tap: 150 times)."""
import numpy as np
import pytest
import torch

import head_ref as HR

CASES = [(preset, size, batch, nc) for preset in ("v1", "v2") for size, batch, nc in ((320, 5, 1), (352, 2, 3))]
PER_IMAGE, CONF = 8, 0.25


_BUILT = {}


def _ids(p):
    return f"{p[0]}-{p[1]}x{p[2]}-nc{p[3]}"


@pytest.fixture(scope="module", params=CASES, ids=_ids)
def case(request, tmp_path_factory):
    return _build(request.param, tmp_path_factory)


@pytest.fixture(scope="module", params=[c for c in CASES if c[3] >= 3], ids=_ids)
def case_nc3(request, tmp_path_factory):
    return _build(request.param, tmp_path_factory)


def _build(param, tmp_path_factory):
    """Model, oracle blobs and the reference pair of every level, computed once per case and shared (read-only)."""
    if param not in _BUILT:
        _BUILT[param] = _build_case(param, tmp_path_factory)
    return _BUILT[param]


def _build_case(param, tmp_path_factory):
    from litepi import ncnn_export
    from oracle import ncnn_ref
    preset, S, BATCH, nc = param
    d = tmp_path_factory.mktemp(f"headref_{preset}_{S}_{nc}")
    p, b = str(d / "m.param"), str(d / "m.bin")
    ncnn_export.export_detector(p, b, preset, seed=6400 + S + nc, nc=nc, cls_bias=0.0, size=S)
    imgs = np.random.default_rng(11 * S + nc).integers(0, 256, (BATCH, S, S, 3), dtype=np.uint8)
    x = torch.from_numpy(imgs[..., ::-1].astype(np.float32) * np.float32(1 / 255.0)).permute(0, 3, 1, 2).contiguous()
    s = np.sort(ncnn_ref.run_graph(ncnn_ref.load_model(p, b), x)["out0"].numpy()[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    k = PER_IMAGE * BATCH
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(CONF / (1 - CONF)) - mid), nc=nc)
    layers = ncnn_ref.load_model(p, b)
    heads = HR.find_heads(layers)
    assert len(heads) == 3
    blobs = ncnn_ref.run_graph(layers, x, keep=["out0"] + [h["feat"] for h in heads])
    anchors, strides = ncnn_export.make_anchors(S)
    dfl = np.arange(16, dtype=np.float64)
    levels, off = [], 0
    for h in heads:
        feat32 = blobs[h["feat"]].numpy()
        H, W = feat32.shape[2:]
        lv = dict(head=h, feat32=feat32, off=off, n=H * W, H=H, W=W, anchors=anchors[:, off:off + H * W], stride=float(strides[off]))
        # the map as a device holds it (fp16-exact), the reference pair on it and the stand-in kernel
        lv["feat"] = HR.round_fp16(torch.from_numpy(feat32)).numpy()
        args = (lv["feat"], h, lv["anchors"], lv["stride"], dfl)
        lv["exact"] = HR.head_out0(*args, round_mid=False, round_logits=False)
        lv["emul"] = HR.head_out0(*args, round_mid=True, round_logits=False)
        lv["standin"] = HR.standin_out0(*args)
        levels.append(lv)
        off += H * W
    assert off == anchors.shape[1] == blobs["out0"].shape[2]
    return dict(preset=preset, S=S, nc=nc, out0=blobs["out0"].numpy(), levels=levels, dfl=dfl)


def test_find_heads_shapes(case):
    nc, c3 = case["nc"], {"v1": 32, "v2": 48}[case["preset"]]
    for lv, stride in zip(case["levels"], (8, 16, 32)):
        h = lv["head"]
        assert lv["H"] == case["S"] // stride and lv["stride"] == stride
        assert [L.weight.shape[0] for L in h["box"]] == [64, 64, 64] and [L.weight.shape[0] for L in h["cls"]] == [c3, c3, nc]
        assert h["box"][0].weight.shape[1] == h["cls"][0].weight.shape[1] == lv["feat32"].shape[1]


def test_reference_equals_the_oracle_graph(case):
    """fp32 weights, no rounding, the oracle's own fp32 neck blobs: the oracle's out0, within the bound the suite uses between an fp32
    implementation and the fp32 oracle (measured: ~1e-5)."""
    worst = 0.0
    for lv in case["levels"]:
        got = HR.head_out0(lv["feat32"], lv["head"], lv["anchors"], lv["stride"], case["dfl"], round_mid=False, round_logits=False,
                           round_weights=False)
        want = case["out0"][:, :, lv["off"]:lv["off"] + lv["n"]].astype(np.float64)
        assert got.shape == want.shape and got.dtype == np.float64
        err = np.abs(got - want)
        worst = max(worst, float(err.max()))
        assert (err <= 1e-3 + 1e-3 * np.abs(want)).all(), f"level {lv['H']}: max err {err.max():.3e}"
    print(f"{case['preset']} {case['S']} nc {case['nc']}: float64 head vs the fp32 oracle's out0: max abs err {worst:.2e}")
    assert worst < 1e-3


def test_budget_holds_for_a_stand_in_kernel(case):
    """The caps of test_gpu_head_float64.py, for the reference alone: an fp32 head with another K order and fp16 intermediates stays
    within 2 max(e) per element and MEAN_CAP mean(e) on average, and the budget e is not vacuous."""
    for lv in case["levels"]:
        st = HR.measure(lv["standin"], lv["exact"], lv["emul"], lv["stride"])
        print(f"{case['preset']} {case['S']} nc {case['nc']} level {lv['H']}: {HR.fmt(st)}")
        for k, s in st.items():
            assert s["max_e"] >= HR.MIN_MAX_E[k], f"level {lv['H']} {k}: max e {s['max_e']:.2e}: the budget is vacuous"
        assert not HR.broken_caps(st, HR.MEAN_CAP), f"level {lv['H']}: {HR.broken_caps(st, HR.MEAN_CAP)}"


def test_round_logits_is_a_rounding_point_of_its_own(case):
    """The three-launch plan's fp16 projections: the stand-in that rounds them stays within the caps of the emulation that rounds them too."""
    for lv in case["levels"]:
        args = (lv["feat"], lv["head"], lv["anchors"], lv["stride"], case["dfl"])
        emul = HR.head_out0(*args, round_mid=True, round_logits=True)
        st = HR.measure(HR.standin_out0(*args, round_logits=True), lv["exact"], emul, lv["stride"])
        print(f"{case['preset']} {case['S']} nc {case['nc']} level {lv['H']} (fp16 logits): {HR.fmt(st)}")
        assert not HR.broken_caps(st, HR.MEAN_CAP), f"level {lv['H']}: {HR.broken_caps(st, HR.MEAN_CAP)}"


CLASS_MUTATIONS = ("cls_swap12", "cls_bias21")   # need classes 1 and 2


@pytest.mark.parametrize("mutation", [m for m in HR.MUTATIONS if m not in CLASS_MUTATIONS])
def test_every_mutation_breaks_a_cap(case, mutation):
    """Each deliberate error of the emulated reference breaks at least one cap on every level it touches, measured against the
    (correct) stand-in kernel and the budget of the unmutated pair."""
    _mutation_breaks_a_cap(case, mutation)


@pytest.mark.parametrize("mutation", CLASS_MUTATIONS)
def test_every_class_mutation_breaks_a_cap(case_nc3, mutation):
    _mutation_breaks_a_cap(case_nc3, mutation)


def _mutation_breaks_a_cap(case, mutation):
    touched = 0
    for lv in case["levels"]:
        if (mutation == "box2_tap02_col15" and lv["W"] < 16) or (mutation == "box2_tap02_row9" and lv["H"] < 10):
            continue   # no such column / row on this map
        mut = HR.head_out0(lv["feat"], lv["head"], lv["anchors"], lv["stride"], case["dfl"], round_mid=True, round_logits=False, mutate=mutation)
        st = HR.measure(lv["standin"], lv["exact"], mut, lv["stride"])
        e = HR.measure(lv["standin"], lv["exact"], lv["emul"], lv["stride"])
        for k in st:   # the budget is the unmutated pair's
            st[k]["max_e"], st[k]["mean_e"] = e[k]["max_e"], e[k]["mean_e"]
        broken = HR.broken_caps(st, HR.MEAN_CAP)
        print(f"{case['preset']} {case['S']} nc {case['nc']} level {lv['H']} {mutation}: {HR.fmt(st)}")
        assert broken, f"level {lv['H']}: {mutation} stays within both caps"
        touched += 1
    assert touched >= 2
