"""GPU tests that pin every fp16 launch of c2f_kernels.hip -- the whole-C2f configurations, the stride-2 kernels and the one-launch
SPPF -- to a float64 reference of ITS OWN HBM INPUT: given the blobs a launch reads (``debug_blob``), does it write the right
output blob?  The end-to-end fp16 bound (test_gpu_parity.py) absorbs the rounding of 20+ layers and the plan-against-plan
comparison allows 1.25x plus a floor; one wrong halo tap on one tile edge, one channel block or the last image of a batch
moves out0 by far less.  test_gpu_head_float64.py pins the Detect head the same way; this module pins what lies between the stem
blocks and the head wherever c2f_kernels.hip runs it.

Per launch whose name starts with c2f<, s2conv or sppf<, with tests/c2f_ref.py on the device's own cut blobs:
    R_exact = float64 span, fp16 weights, nothing else rounded
    R_emul  = the same with the kernel's rounding points (every Swish output, every add output)
    e = |R_emul - R_exact|   what fp16 storage itself costs -- CPU only, nothing of the code under test
    d = |got - R_emul|
Asserts: every d <= 2 max(e); mean(d) <= MEAN_CAP mean(e) (0.5); max(e) >= 2**-11; every blob finite, fp16-exact, std > 0.05; the
launches a case names are in its profile.  test_c2f_ref_cpu.py shows that a correct implementation with another summation order
stays within the caps and that a dropped halo tap, exchanged concat segments or images, a skipped shortcut, a shifted upsample,
a wrong padding tap and a short pool window break them.  A ratio above the caps is a finding -- a rounding point c2f_ref.py lacks,
or a bug: name it from the kernel's code, do not widen a cap.

Cases: v1 and v2 (export_detector(preset, seed=77, cls_bias=-2.0)) at 640 x 640 -- the smallest size at which the configurations
run on more than one tile (80 x 80: 5 x 4 tiles of 16 x 20; 40 x 40: 2 x 2 tiles or 4 x 2 of 10 x 20; 20 x 20: two half-image
tiles) and at which the whole-image configurations and sppf<192,96,192> exist --, an fp16 handle of capacity 4 holding 3 images,
all images compared; the planner's switches that reach the other configurations (CASES).  Every plan-time switch of
c2f_kernels.hip, LITEPI_NO_S2TAIL among them, is read per load (PlanSwitches, detector_plan.cpp):
test_switches_are_read_per_load pins that with three loads in this process; the c2f<16,2,32> case keeps the child process it was
written with.  test_no_s2c_alone_on_v2 pins the plan of LITEPI_NO_S2C=1 alone on v2, whose load once claimed cv1 as the tail of a
launch the switch forbids.  One further test per preset runs the bisect mode (LITEPI_C2F_STORE_ALL=1): out0
byte-equal to the production run, and every intermediate the modules then store within the same two caps.

MEAN_CAP (tests/c2f_ref.py) = 0.5 comes from the CPU stand-in (test_c2f_ref_cpu.py), not from the figures below.  MI355X, this
module as committed, over all 95 launch rows of the ten tests (87 of the first eight, unchanged by the move of the switches into the
planner, and the 8 of test_no_s2c_alone_on_v2: at most 1.387 and 0.1561 there): largest max d / max e 1.761 (c2f<96,1,288> behind
LITEPI_NO_C2F_XCV1, cap 2), largest mean d / mean e 0.4345 (c2f<64,1,s2+128,sppf> behind LITEPI_C2F_XCV1; the stand-in measures
0.41 on that span: one flipped rounding of s spreads through three 5 x 5 pools), smallest max e 1.84e-3 (floor 4.9e-4).  Bisect
mode, 49 intermediates: largest max d / max e 1.098 and mean d / mean e 0.216 (SPPF's s of c2f<64,1,s2+128,sppf>); out0 byte-equal.
Every configuration the cases name is reachable: c2f<16,2,32> is planned under LITEPI_C2F_BB80=1 LITEPI_NO_S2TAIL=1.
Rows of the launches a case names (the other launches of a switched case repeat the production rows on slightly different inputs):
    case       launch                 layer                              max e    mean e     max d    mean d  d/e max   mean   equal
    v1         s2conv+1x1<16,32>      conv_6+conv_7                   2.93e-03  1.13e-04  3.91e-03  1.88e-07    1.334  0.0017  99.88%
    v1         s2conv<32,64>          conv_13                         1.84e-03  7.44e-05  1.95e-03  4.57e-08    1.059  0.0006  99.94%
    v1         c2f<32,2,64>           conv_14..conv_19                3.56e-03  1.83e-04  3.91e-03  2.08e-05    1.097  0.1134  89.68%
    v1         c2f<64,1,s2+128,sppf>  conv_20+conv_21..conv_24+sppf   2.25e-03  1.78e-04  1.95e-03  6.28e-05    0.868  0.3530  67.59%
    v1         c2f<32,1,up128+64>     conv_27..conv_30                4.37e-03  1.73e-04  3.91e-03  5.70e-06    0.894  0.0330  97.11%
    v1         c2f<16,1,up64+32>      conv_31..conv_34                5.75e-03  1.60e-04  3.91e-03  1.61e-06    0.679  0.0101  99.01%
    v1         s2conv<32,64>          conv_35                         3.07e-03  8.04e-05  1.95e-03  6.04e-08    0.637  0.0008  99.94%
    v1         c2f<32,1,128>          conv_36..conv_39                7.55e-03  1.87e-04  7.81e-03  3.37e-06    1.034  0.0180  98.17%
    v1         c2f<64,1,s2+256>       conv_40+conv_41..conv_44        7.46e-03  1.95e-04  7.81e-03  2.64e-05    1.048  0.1359  86.96%
    v1-xcv1    c2f<16,2,y0y1>         conv_8..conv_12                 3.09e-03  1.59e-04  3.91e-03  2.97e-06    1.264  0.0187  98.39%
    v1-skip20  s2conv<64,128>         conv_20                         1.94e-03  7.92e-05  1.95e-03  6.32e-08    1.009  0.0008  99.93%
    v1-skip20  c2f<64,1,128>          conv_21..conv_24                3.55e-03  1.82e-04  3.91e-03  1.13e-05    1.101  0.0620  93.97%
    v1-skip20  s2conv<64,128>         conv_40                         3.89e-03  7.59e-05  9.77e-04  5.75e-08    0.251  0.0008  99.92%
    v1-skip20  c2f<64,1,256>          conv_41..conv_44                1.05e-02  1.79e-04  7.81e-03  9.11e-06    0.743  0.0509  94.78%
    v2         s2conv+1x1<24,48>      conv_6+conv_7                   2.92e-03  1.22e-04  1.95e-03  2.54e-07    0.668  0.0021  99.81%
    v2         c2f<24,2,y0y1>         conv_8..conv_12                 3.27e-03  1.37e-04  3.91e-03  5.44e-06    1.196  0.0397  96.56%
    v2         s2conv<48,96>          conv_13                         1.92e-03  6.33e-05  9.77e-04  4.25e-08    0.508  0.0007  99.94%
    v2         c2f<48,2,96>           conv_14..conv_19                3.65e-03  1.78e-04  3.91e-03  3.08e-05    1.071  0.1732  83.80%
    v2         s2conv<96,192>         conv_20                         1.95e-03  7.50e-05  1.95e-03  5.89e-08    1.001  0.0008  99.91%
    v2         c2f<96,1,192>          conv_21..conv_24                2.82e-03  1.47e-04  3.91e-03  1.01e-05    1.384  0.0687  93.53%
    v2         sppf<192,96,192>       conv_25+pools+conv_26           2.31e-03  1.31e-04  1.95e-03  1.41e-07    0.845  0.0011  99.89%
    v2         c2f<48,1,up192+96>     conv_27..conv_30                4.51e-03  1.82e-04  3.91e-03  8.15e-06    0.867  0.0448  95.68%
    v2         c2f<24,1,up96+48>      conv_31..conv_34                4.57e-03  1.59e-04  3.91e-03  1.73e-06    0.854  0.0109  99.00%
    v2         s2conv<48,48>          conv_35                         3.78e-03  9.23e-05  1.95e-03  9.49e-08    0.516  0.0010  99.93%
    v2         c2f<48,1,144>          conv_36..conv_39                5.18e-03  2.13e-04  3.91e-03  8.93e-06    0.754  0.0420  95.98%
    v2         s2conv<96,96>          conv_40                         3.28e-03  9.33e-05  1.95e-03  7.28e-08    0.595  0.0008  99.91%
    v2         c2f<96,1,288>          conv_41..conv_44                7.34e-03  2.18e-04  7.81e-03  1.84e-05    1.064  0.0843  91.86%
    v2-no_xcv1 s2conv<24,48>          conv_6                          1.94e-03  6.78e-05  1.95e-03  4.28e-08    1.006  0.0006  99.95%
    v2-no_xcv1 c2f<24,2,48>           conv_7..conv_12                 3.51e-03  1.55e-04  3.91e-03  1.06e-05    1.114  0.0680  93.70%
    v1-bb80    c2f<16,2,32>           conv_7..conv_12                 3.12e-03  1.85e-04  3.91e-03  6.67e-06    1.251  0.0360  96.54%
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import c2f_ref as CR
from test_c2f_ref_cpu import BATCH, S, SPANS, images

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 4
SWITCHES = ("LITEPI_NO_C2F", "LITEPI_NO_S2C", "LITEPI_C2F_XCV1", "LITEPI_NO_C2F_XCV1", "LITEPI_C2F_SKIP", "LITEPI_C2F_STORE_ALL",
            "LITEPI_C2F_BB80", "LITEPI_NO_S2TAIL", "LITEPI_C2F_MIN_BATCH", "LITEPI_NO_S2LDS", "LITEPI_NO_SPPF_FUSED")
_SKIP_20x20 = "c2f<64,1,s2+256>;c2f<64,1,s2+128,sppf>"
# case -> (preset, switches, the launches its profile must hold: name -> count)
CASES = {
    "v1": ("v1", {}, {"c2f<32,2,64>": 1, "c2f<64,1,s2+128,sppf>": 1, "c2f<32,1,up128+64>": 1, "c2f<16,1,up64+32>": 1, "c2f<32,1,128>": 1,
                      "c2f<64,1,s2+256>": 1, "s2conv+1x1<16,32>": 1, "s2conv<32,64>": 2}),
    "v1-xcv1": ("v1", {"LITEPI_C2F_XCV1": "1"}, {"c2f<16,2,y0y1>": 1}),
    "v1-skip20": ("v1", {"LITEPI_C2F_SKIP": _SKIP_20x20}, {"c2f<64,1,128>": 1, "c2f<64,1,256>": 1, "s2conv<64,128>": 2}),
    "v2": ("v2", {}, {"c2f<24,2,y0y1>": 1, "c2f<48,2,96>": 1, "c2f<96,1,192>": 1, "sppf<192,96,192>": 1, "c2f<48,1,up192+96>": 1,
                      "c2f<24,1,up96+48>": 1, "c2f<48,1,144>": 1, "c2f<96,1,288>": 1, "s2conv+1x1<24,48>": 1, "s2conv<48,96>": 1,
                      "s2conv<96,192>": 1, "s2conv<48,48>": 1, "s2conv<96,96>": 1}),
    "v2-no_xcv1": ("v2", {"LITEPI_NO_C2F_XCV1": "1"}, {"c2f<24,2,48>": 1, "s2conv<24,48>": 1}),
}
CHILD_CASE = ("v1", {"LITEPI_C2F_BB80": "1", "LITEPI_NO_S2TAIL": "1"}, {"c2f<16,2,32>": 1})
_MODELS, _PRODUCTION = {}, {}


def _model(preset, tmp_path_factory):
    if preset not in _MODELS:
        from litepi import ncnn_export
        from oracle import ncnn_ref
        d = tmp_path_factory.mktemp(f"c2f64_{preset}")
        p, b = str(d / "m.param"), str(d / "m.bin")
        ncnn_export.export_detector(p, b, preset, seed=77, cls_bias=-2.0)
        imgs_path = str(d / "imgs.npy")
        np.save(imgs_path, images())
        _MODELS[preset] = dict(p=p, b=b, layers=ncnn_ref.load_model(p, b), imgs=images(), imgs_path=imgs_path)
    return _MODELS[preset]


def _is_ours(name):
    return name.startswith(("c2f<", "s2conv", "sppf<"))


def _intermediates(layers, sp, name):
    """What a c2f< launch stores in the bisect mode besides its output: the Slice outputs y0 and y1, every add output, the entry
    conv's x, the C2f output and SPPF's s where the SPPF follows in the launch, and the pooled maps."""
    if not name.startswith("c2f<"):
        return []
    prod = {o: L for L in layers for o in L.outputs}
    sliced = {L.inputs[0] for L in sp["inside"] if L.type == "Slice"}
    out = []
    for L in sp["inside"]:
        if L.type in ("Slice", "BinaryOp", "Pooling"):
            out += list(L.outputs)
        elif L.type == "Swish" and L.outputs[0] != sp["out"] and L.outputs[0] not in sliced:
            c = prod[L.inputs[0]]
            if int(c.params.get(3, 1)) == 2 or int(c.params.get(1, 1)) == 1:
                out.append(L.outputs[0])
    return out


def _run(m, env, monkeypatch, want_intermediates=False):
    """One fp16 engine on the case: out0 of detect_raw, the launches of the profile (the second call) and, for each of ours, its cut
    blobs and output blob (and the stored intermediates) of all three images; a refusal is kept as its message."""
    from litepi import Engine
    from litepi._ffi import LitepiError
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # the planner reads its switches when the model is loaded
    e = Engine(precision="fp16", max_batch=CAP, max_det=300, det_input=S)
    try:
        e.load_detector(m["p"], m["b"])
        out0 = np.array(e.detect_raw(m["imgs"]))
        e.profile_next(True)
        out0b = np.array(e.detect_raw(m["imgs"]))
        launches = [(k["name"], k["layer"]) for k in e.profile_read()]
        blobs = {}
        for name, ls in launches:
            if not _is_ours(name):
                continue
            sp = CR.span(m["layers"], CR.launch_convs(ls, m["layers"]))
            for b in sp["cuts"] + [sp["out"]] + (_intermediates(m["layers"], sp, name) if want_intermediates else []):
                if b not in blobs:
                    try:
                        blobs[b] = e.debug_blob(b, batch=BATCH)
                    except LitepiError as err:
                        blobs[b] = str(err)
    finally:
        e.close()
    assert (out0 == out0b).all(), "two calls on the same images differ"
    return out0, launches, blobs


def _blob_ok(blobs, b, failures, tag):
    v = blobs.get(b)
    if not isinstance(v, np.ndarray):
        # the tensor is in HBM: a refusal is a defect of Detector::fetch_blob or of the planner's in_c2f / materialised marks
        failures.append(f"{tag}: blob {b} refused: {v}")
        return False
    if not (np.isfinite(v).all() and (v == v.astype(np.float16)).all() and v.shape[0] == BATCH):
        failures.append(f"{tag}: blob {b} is not finite and fp16-exact")
        return False
    if not v.std() > 0.05:
        failures.append(f"{tag}: blob {b} looks unwritten (std {v.std():.3g})")
        return False
    return True


def _check(m, case, out0, launches, blobs, required, want_intermediates=False):
    """Every launch of ours against the float64 reference of its own cut blobs; all failures of a case in one message."""
    assert np.isfinite(out0).all()
    names = [n for n, _ in launches]
    for want, count in required.items():
        assert names.count(want + "_f16") == count, f"{case}: {want} x {count} expected in the profile: {names}"
    failures = []
    for name, ls in launches:
        if not _is_ours(name):
            continue
        tag = f"{case} {name} {ls}"
        assert ls in SPANS, f"{tag}: not in the table of test_c2f_ref_cpu.py"
        convs = CR.launch_convs(ls, m["layers"])
        sp = CR.span(m["layers"], convs)
        if not all([_blob_ok(blobs, b, failures, tag) for b in sp["cuts"] + [sp["out"]]]):
            continue
        ins = {c: blobs[c] for c in sp["cuts"]}
        keep = [b for b in _intermediates(m["layers"], sp, name)] if want_intermediates else []
        exact, kx = CR.eval_span(m["layers"], convs, ins, round_act=False, keep=keep + [sp["out"]])
        emul, km = CR.eval_span(m["layers"], convs, ins, round_act=True, keep=keep + [sp["out"]])
        st = CR.measure(blobs[sp["out"]], exact, emul)
        print(f"{case:10s} {name:28s} {ls:30s} {CR.fmt(st)}")
        failures += [f"{tag}: {f}" for f in CR.check(st)]
        for b in keep:   # bisect mode: a failing launch names its first wrong phase
            if not _blob_ok(blobs, b, failures, tag):
                continue
            sb = CR.measure(blobs[b], kx[b], km[b])
            a = sb["act"]
            print(f"{case:10s} {name:28s}   blob {b:4s} max e {a['max_e']:.2e} mean e {a['mean_e']:.2e} max d {a['max_d']:.2e} mean d {a['mean_d']:.2e} "
                  f"equal {100 * a['equal']:.2f}%")
            failures += [f"{tag}: blob {b}: {f}" for f in CR.broken_caps(sb, CR.MEAN_CAP)]
    assert not failures, " | ".join(failures)


@pytest.mark.parametrize("case", list(CASES))
def test_launch_equals_float64_reference_of_its_input(case, tmp_path_factory, monkeypatch):
    preset, env, required = CASES[case]
    m = _model(preset, tmp_path_factory)
    out0, launches, blobs = _run(m, env, monkeypatch)
    if not env:
        _PRODUCTION[preset] = out0
    _check(m, case, out0, launches, blobs, required)


@pytest.mark.parametrize("preset", ["v1", "v2"])
def test_bisect_mode_stores_what_the_modules_compute(preset, tmp_path_factory, monkeypatch):
    """LITEPI_C2F_STORE_ALL=1 set before the load (the switch tools/c2f_check.py and the A/B scripts rely on): out0 byte-equal to the
    production run of the same case, the same launches, and every intermediate the modules then store -- y0, y1, each bottleneck's
    add output, the entry conv's x, the C2f output, SPPF's s and the three pooled maps of c2f<64,1,s2+128,sppf> -- within the two caps
    against eval_span(keep=...)."""
    m = _model(preset, tmp_path_factory)
    if preset not in _PRODUCTION:
        _PRODUCTION[preset] = _run(m, {}, monkeypatch)[0]
    out0, launches, blobs = _run(m, {"LITEPI_C2F_STORE_ALL": "1"}, monkeypatch, want_intermediates=True)
    assert out0.tobytes() == _PRODUCTION[preset].tobytes(), "the bisect mode changes out0"
    _check(m, preset + "-bisect", out0, launches, blobs, CASES[preset][2], want_intermediates=True)
    if preset == "v1":   # the whole-image launch stores x, y0, y1, the add, the C2f output, s and the three pooled maps
        assert all(isinstance(blobs.get(b), np.ndarray) for b in ("75", "78", "79", "87", "90", "92", "95", "98", "101")), sorted(blobs)


def test_switches_are_read_per_load(tmp_path_factory, monkeypatch):
    """Three loads of v1 in this process -- no switch, LITEPI_NO_S2TAIL=1, no switch: the stride-2 launch with its 1x1 tail is in the
    first and third profiles and not in the second, and the first and third out0 are equal byte for byte.  (The switch used to be a
    static of c2f_kernels.hip, latched by the first load of the process.)"""
    m = _model("v1", tmp_path_factory)
    runs = [_run(m, env, monkeypatch) for env in ({}, {"LITEPI_NO_S2TAIL": "1"}, {})]
    has_tail = ["s2conv+1x1<16,32>_f16" in [n for n, _ in launches] for _, launches, _ in runs]
    assert has_tail == [True, False, True], [[n for n, _ in launches if _is_ours(n)] for _, launches, _ in runs]
    assert runs[0][0].tobytes() == runs[2][0].tobytes(), "out0 of the two loads without a switch differ"


def test_no_s2c_alone_on_v2(tmp_path_factory, monkeypatch):
    """LITEPI_NO_S2C=1 and no other switch on v2: the load succeeds, no stride-2 launch of c2f_kernels.hip is planned -- so cv1 of
    the 80 x 80 module is not claimed as the tail of one either (the planner once claimed it without asking this switch and failed
    the load in ConvLayer::attach_tail) --, and every remaining c2f< / sppf< launch stays within the two caps."""
    m = _model("v2", tmp_path_factory)
    out0, launches, blobs = _run(m, {"LITEPI_NO_S2C": "1"}, monkeypatch)
    names = [n for n, _ in launches]
    print("LITEPI_NO_S2C=1 v2:", [n for n in names if _is_ours(n)])
    assert not [n for n in names if n.startswith("s2conv")], names
    assert [n for n in names if n.startswith("c2f<")], names   # (the checks below are not vacuous)
    _check(m, "v2-no_s2c", out0, launches, blobs, {})


# A fresh process for the case that was written when LITEPI_NO_S2TAIL was latched per process (it is read per load now; the case
# stays as it was): out0, the launches and every blob of the table the plan hands out -> .npz
_CHILD = r"""
import sys
import numpy as np
from litepi import Engine
from litepi._ffi import LitepiError
p, b, imgs_path, out, S, B, cap = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7])
imgs = np.load(imgs_path)
e = Engine(precision="fp16", max_batch=cap, max_det=300, det_input=S)
try:
    e.load_detector(p, b)
    res = {"out0": np.array(e.detect_raw(imgs))}
    for name in sys.argv[8:]:
        try:
            res["blob_" + name] = e.debug_blob(name, batch=B)
        except LitepiError as err:
            res["refused_" + name] = np.array(str(err))
    e.profile_next(True)
    e.detect_raw(imgs)
    prof = e.profile_read()
    res["names"] = np.array([k["name"] for k in prof])
    res["layers"] = np.array([k["layer"] for k in prof])
finally:
    e.close()
np.savez(out, **res)
"""


def test_bb80_module_equals_float64_reference(tmp_path_factory, tmp_path):
    """c2f<16,2,32>, the opt-in n = 2 module on the 80 x 80 map: LITEPI_C2F_BB80=1 enables it and LITEPI_NO_S2TAIL=1 keeps its cv1
    out of the stride-2 launch in front."""
    preset, switches, required = CHILD_CASE
    m = _model(preset, tmp_path_factory)
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "yolo-litepi_amd"), ROOT, env.get("PYTHONPATH", "")])
    env.update(switches)
    out = tmp_path / "out.npz"
    table = sorted({b for cuts, o in SPANS.values() for b in cuts + [o]}, key=int)
    r = subprocess.run([sys.executable, "-c", _CHILD, m["p"], m["b"], m["imgs_path"], str(out), str(S), str(BATCH), str(CAP)] + table,
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as z:
        out0 = z["out0"]
        launches = [(str(n), str(ls)) for n, ls in zip(z["names"], z["layers"])]
        blobs = {k[5:]: z[k] for k in z.files if k.startswith("blob_")}
        blobs.update({k[8:]: str(z[k]) for k in z.files if k.startswith("refused_")})
    _check(m, "v1-bb80", out0, launches, blobs, required)
