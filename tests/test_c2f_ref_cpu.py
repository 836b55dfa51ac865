"""CPU tests of tests/c2f_ref.py, the float64 restatement of a launch's span of the graph that test_gpu_c2f_float64.py holds the
fp16 launches of c2f_kernels.hip against: the launch strings of the recorded plans parse into the expected spans, the restatement
computes what the oracle's graph computes, its error budget holds for a correct fp16 implementation that is not the kernel, and
the budget's caps catch the errors a tiled kernel makes.

Cases: the GPU module's models and images (the exporter's v1 and v2 at 640, seed 77, three seeded images), every span of the
table SPANS that is a launch of the preset (15 of v1, 15 of v2); the cut blobs come from the fp32 oracle, rounded to fp16 as a device holds them.

Measured here (this module's own prints, -s):
  float64 spans against the fp32 oracle's blobs: at most 0.036 of the bound 1e-4 + 1e-4 |ref|.
  stand-in kernel: max d / max e <= 1.589 (v2 conv_6+conv_7; cap 2), max e >= 1.86e-3 (floor 2**-11 = 4.9e-4);
    mean d / mean e: 0.4097 on v1's whole-image conv_20+conv_21..conv_24+sppf (seven rounding points in a row, then three 5 x 5 max
    pools on a 20 x 20 map that spread one flipped rounding of s over up to 13 x 13 pixels: 63 % of the output is bit-equal),
    0.2094 on v2 conv_14..conv_19, 0.1573 on v1 conv_40+conv_41..conv_44, below 0.1 on every other span, below 0.002 on the
    single convolutions.  Twice the largest is 0.82, the next power of two 1: MEAN_CAP is the ceiling, 0.5.
  mutations: every one breaks a cap on every span it applies to; the smallest factor over a cap is 38.9 (s2_pad_centre on v1's
    whole-image launch, whose padding taps touch one row and one column of a 20 x 20 map); a dropped halo tap at least 66 times,
    the short pool window 111 and 197 times, exchanged segments / images, the skipped shortcut and the shifted upsample over 900.
  b2_tap02_col19 does not apply to the 20 x 20 maps: column 19 is their last, the dropped tap reads the zero padding.
"""
import json
import os

import numpy as np
import pytest
import torch

import c2f_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, BATCH = 640, 3
PRESETS = ("v1", "v2")
# launch string of a profile / of tests/golden/detector_plans.json -> (cut blobs, output blob); the exporter's v1 and v2 share the graph
SPANS = {
    "conv_6+conv_7": (["19"], "23"),                          # stride-2 conv + C2f.cv1 as its 1x1 tail
    "conv_6": (["19"], "21"),
    "conv_7..conv_12": (["21"], "44"),
    "conv_8..conv_12": (["23"], "44"),                        # cv1-less module: reads cv1's y0 | y1
    "conv_13": (["44"], "48"),
    "conv_14..conv_19": (["48"], "71"),
    "conv_20": (["71"], "75"),
    "conv_21..conv_24": (["75"], "90"),
    "conv_20+conv_21..conv_24+sppf": (["71"], "104"),         # stride-2 conv + C2f + SPPF, whole image
    "conv_25+pools+conv_26": (["90"], "104"),
    "conv_27..conv_30": (["71", "104"], "123"),               # P4 and the half-resolution P5 of the fused upsample
    "conv_31..conv_34": (["44", "123"], "142"),               # P3 and the half-resolution F4
    "conv_35": (["142"], "147"),
    "conv_36..conv_39": (["123", "147"], "163"),              # F4 is the second concat operand
    "conv_40": (["163"], "168"),
    "conv_41..conv_44": (["104", "168"], "184"),
    "conv_40+conv_41..conv_44": (["104", "163"], "184"),      # stride-2 conv + C2f; P5 is the second concat operand
}
# the spans that are launches of a preset: those its recorded plans hold, and for v1 the pair of c2f<16,2,32> (LITEPI_C2F_BB80=1
# LITEPI_NO_S2TAIL=1), which no recorded plan holds.  v1 alone has the whole-image configurations, v2 alone the one-launch SPPF.
ONLY = {"v1": ("conv_20+conv_21..conv_24+sppf", "conv_40+conv_41..conv_44"), "v2": ("conv_25+pools+conv_26",)}
_BUILT = {}


def spans_of(preset):
    other = [ls for p, v in ONLY.items() if p != preset for ls in v]
    return [ls for ls in SPANS if ls not in other]


def images():
    return np.random.default_rng(640077).integers(0, 256, (BATCH, S, S, 3), dtype=np.uint8)


def _build(preset, tmp_path_factory):
    """Model, the oracle's blobs and, per span, the reference pair and the stand-in: computed once per preset and shared (read-only)."""
    if preset in _BUILT:
        return _BUILT[preset]
    from litepi import ncnn_export
    from oracle import ncnn_ref
    d = tmp_path_factory.mktemp(f"c2fref_{preset}")
    p, b = str(d / "m.param"), str(d / "m.bin")
    ncnn_export.export_detector(p, b, preset, seed=77, cls_bias=-2.0)
    layers = ncnn_ref.load_model(p, b)
    x = torch.from_numpy(images()[..., ::-1].astype(np.float32) * np.float32(1 / 255.0)).permute(0, 3, 1, 2).contiguous()
    names = sorted({n for cuts, out in SPANS.values() for n in cuts + [out]})
    blobs = {k: v.numpy() for k, v in ncnn_ref.run_graph(layers, x, keep=names).items()}
    spans = {}
    for ls in spans_of(preset):
        convs = CR.launch_convs(ls, layers)
        sp = CR.span(layers, convs)
        ins = {c: CR.round_fp16(torch.from_numpy(blobs[c])).numpy() for c in sp["cuts"]}
        spans[ls] = dict(convs=convs, span=sp, ins=ins,
                         exact=CR.eval_span(layers, convs, ins, round_act=False),
                         emul=CR.eval_span(layers, convs, ins, round_act=True),
                         standin=CR.standin_span(layers, convs, ins))
    _BUILT[preset] = dict(preset=preset, layers=layers, blobs=blobs, spans=spans)
    return _BUILT[preset]


@pytest.fixture(scope="module", params=PRESETS)
def case(request, tmp_path_factory):
    return _build(request.param, tmp_path_factory)


def test_every_recorded_launch_parses_into_its_span(case):
    """Every c2f< / s2conv / sppf< entry of the recorded v1 and v2 plans: the string parses, and the span's cut blobs and output blob
    are those of the table."""
    with open(os.path.join(ROOT, "tests", "golden", "detector_plans.json")) as f:
        plans = json.load(f)
    seen = set()
    for key, plan in plans.items():
        if not key.startswith(case["preset"] + "-"):
            continue
        for name, ls, *_ in plan["launches"]:
            if name.startswith(("c2f<", "s2conv", "sppf<")):
                assert ls in SPANS, f"{key}: {name} {ls}: not in the table"
                sp = CR.span(case["layers"], CR.launch_convs(ls, case["layers"]))
                assert (sp["cuts"], sp["out"]) == SPANS[ls], f"{key}: {name} {ls}: {sp['cuts']} -> {sp['out']}"
                seen.add(ls)
    assert len(seen) >= 13, sorted(seen)
    assert seen <= set(spans_of(case["preset"])), sorted(seen)
    for ls, s in case["spans"].items():
        assert (s["span"]["cuts"], s["span"]["out"]) == SPANS[ls], ls
    # the never-written upsampled concat segment is not a cut blob; the half-resolution source is
    assert "107" not in SPANS["conv_27..conv_30"][0] and "126" not in SPANS["conv_31..conv_34"][0]
    with pytest.raises(AssertionError):
        CR.launch_convs("conv_45|conv_48+conv_46+conv_47", case["layers"])


def test_unrounded_reference_equals_the_oracle_graph(case):
    """fp32 weights, no rounding, the oracle's own fp32 cut blobs: the oracle's blob within 1e-4 + 1e-4 |ref| (fp32 noise of the oracle)."""
    worst = 0.0
    for ls, s in case["spans"].items():
        got = CR.eval_span(case["layers"], s["convs"], {c: case["blobs"][c] for c in s["span"]["cuts"]}, round_act=False, round_weights=False)
        want = case["blobs"][s["span"]["out"]].astype(np.float64)
        assert got.shape == want.shape and got.dtype == np.float64
        err = np.abs(got - want)
        worst = max(worst, float((err / (1e-4 + 1e-4 * np.abs(want))).max()))
        assert (err <= 1e-4 + 1e-4 * np.abs(want)).all(), f"{ls}: max err {err.max():.3e}"
    print(f"{case['preset']}: float64 spans against the fp32 oracle: worst err / bound {worst:.3f}")


def test_budget_holds_for_a_stand_in_kernel(case):
    """The caps of test_gpu_c2f_float64.py, for the reference alone: fp32 sums in another order with the same fp16 rounding points stay
    within 2 max(e) per element and MEAN_CAP mean(e) on average, and the budget e is above its floor, on every span."""
    failures = []
    for ls, s in case["spans"].items():
        st = CR.measure(s["standin"], s["exact"], s["emul"])
        print(f"standin {case['preset']} {ls:32s} {CR.fmt(st)}")
        failures += [f"{ls}: {m}" for m in CR.check(st)]
    assert not failures, " | ".join(failures)


def test_mean_cap_is_the_power_of_two_the_stand_in_points_at(tmp_path_factory):
    """MEAN_CAP: the smallest power of two at or above twice the stand-in's largest mean d / mean e over all spans of both presets,
    never above 0.5."""
    worst = max(st["mean_d"] / st["mean_e"] for p in PRESETS for s in _build(p, tmp_path_factory)["spans"].values()
                for st in [CR.measure(s["standin"], s["exact"], s["emul"])["act"]])
    print(f"stand-in: largest mean d / mean e {worst:.4f}")
    assert CR.MEAN_CAP == min(0.5, 2.0 ** int(np.ceil(np.log2(2 * worst)))), worst


def test_keep_returns_the_named_intermediates(tmp_path_factory):
    case = _build("v1", tmp_path_factory)
    s = case["spans"]["conv_20+conv_21..conv_24+sppf"]
    out, kept = CR.eval_span(case["layers"], s["convs"], s["ins"], round_act=True, keep=("75", "78", "79", "87", "90", "92", "95", "98", "101"))
    assert (out == s["emul"]).all()
    assert kept["75"].shape[1] == 2 * kept["78"].shape[1] == 2 * kept["87"].shape[1] and kept["90"].shape == kept["75"].shape
    assert (kept["95"] >= kept["92"]).all() and (kept["98"] >= kept["95"]).all() and (kept["101"] >= kept["98"]).all()
    assert all((v == v.astype(np.float16)).all() for v in kept.values())


@pytest.mark.parametrize("mutation", CR.MUTATIONS)
def test_every_mutation_breaks_a_cap(case, mutation):
    """Each deliberate error of the emulated reference breaks at least one cap on every span it applies to, measured against the
    (correct) stand-in kernel and the budget of the unmutated pair."""
    touched = 0
    for ls, s in case["spans"].items():
        if mutation not in CR.mutations_for(case["layers"], s["convs"], width=s["emul"].shape[3]):
            continue
        mut = CR.eval_span(case["layers"], s["convs"], s["ins"], round_act=True, mutate=mutation)
        st = CR.measure(s["standin"], s["exact"], mut)
        e = CR.measure(s["standin"], s["exact"], s["emul"])["act"]
        st["act"]["max_e"], st["act"]["mean_e"] = e["max_e"], e["mean_e"]   # the budget is the unmutated pair's
        a = st["act"]
        factor = max(a["max_d"] / (2 * a["max_e"]), a["mean_d"] / (CR.MEAN_CAP * a["mean_e"]))
        print(f"mutation {case['preset']} {ls:32s} {mutation:18s} {CR.fmt(st)} factor {factor:.2f}")
        assert CR.broken_caps(st, CR.MEAN_CAP), f"{ls}: {mutation} stays within both caps"
        touched += 1
    assert touched >= 1
