"""GPU tests that pin the fp16 Detect head to a float64 reference of ITS OWN INPUT: given the neck map a level's head reads from
HBM (``debug_blob``), does the head emit the right ``out0``?  The end-to-end fp16 bound (test_gpu_parity.py) has to absorb the
rounding of 20+ layers in front of the head and is 35 - 400 times wider than what the head itself costs; test_gpu_head_skip.py and
test_gpu_head_split_a.py pin out0 -> candidates -> records.  This module closes the chain: neck map -> out0.

Per level and row group (box rows in grid cells, score rows), with tests/head_ref.py on the device's own map:
    R_exact = float64 head, fp16 weights, nothing else rounded
    R_emul  = the same with the kernel's rounding points (the two post-SiLU activations; the three-launch plan: the projections too)
    e = |R_emul - R_exact|   what fp16 storage itself costs -- CPU only, nothing of the code under test
    d = |got - R_emul|
Asserts: every d <= 2 max(e); mean(d) <= MEAN_CAP mean(e); max(e) >= 1e-4 cells (box) / 1e-5 (scores); every value of the maps is
fp16-exact and finite; the intended plan ran (``head_fused<`` in the profile, or not).  test_head_ref_cpu.py shows that a correct
implementation with another summation order stays within the caps and that a wrong halo tap, swapped channels, a wrong DFL weight,
shifted anchors and exchanged classes or biases break them.

Cases: v1 and v2 at 320 x 320, batch 5, one class (whole-C2f plan; maps 40 / 20 / 10; masked last tile column on P3) and at
352 x 352, batch 2, three classes (layer plan; maps 44 / 22 / 11; masked edges both ways; the best-of-classes path), each on the
fused plan and on the three-launch plan (LITEPI_NO_HEADFUSE=1); v1 at 352 also behind LITEPI_HEAD_A32 / _2WG / _1WG and v2 at 352
behind LITEPI_HEAD_A32 (its three shapes without 16-pixel tiles, which any of the three switches selects), which are read per
load: one child process each, one after another.  All images of a batch are compared.

MEAN_CAP (tests/head_ref.py) = 0.25: the smallest power of two at or above twice the largest mean d / mean e measured on an MI355X
over all cases, levels and row groups below (0.0641: v2-320x5-nc1, fused, P5, box rows; largest on score rows 0.0461), capped at 0.5.
The largest max d / max e is 1.163 (v2-320x5-nc1, three launches, P4, score rows) against the cap of 2; the smallest max e is
7.59e-4 cells and 6.75e-5 in score.  The stand-in kernel of test_head_ref_cpu.py measures at most 0.93 and 0.10.  A ratio above the
caps is a finding -- a rounding point head_ref.py lacks, or a bug: name it from the kernel's code, do not widen a cap.

MI355X, this module as committed (box rows in grid cells):
    case          plan / switch  level | box: max e   mean e    max d    mean d    d/e max  mean  | score: max e  mean e    max d    mean d    d/e max  mean
    v1-320x5-nc1  fused           40   |    6.21e-03  1.89e-04  2.88e-03  4.69e-06  0.464  0.0248 |    4.56e-04  7.41e-06  1.96e-04  1.29e-07  0.431  0.0174
    v1-320x5-nc1  fused           20   |    8.36e-03  2.41e-04  2.63e-03  8.41e-06  0.315  0.0349 |    4.62e-04  1.09e-05  1.15e-04  2.26e-07  0.249  0.0208
    v1-320x5-nc1  fused           10   |    2.07e-03  1.74e-04  9.72e-04  8.03e-06  0.470  0.0461 |    1.74e-04  6.87e-06  4.61e-06  5.10e-08  0.027  0.0074
    v1-320x5-nc1  three_launch    40   |    7.05e-03  2.40e-04  2.01e-03  7.90e-06  0.285  0.0329 |    4.56e-04  1.60e-05  1.86e-04  1.51e-07  0.408  0.0094
    v1-320x5-nc1  three_launch    20   |    1.05e-02  3.17e-04  4.76e-03  1.91e-05  0.452  0.0601 |    4.61e-04  1.73e-05  3.56e-05  3.73e-08  0.077  0.0022
    v1-320x5-nc1  three_launch    10   |    2.89e-03  2.43e-04  5.89e-04  7.24e-06  0.203  0.0298 |    2.14e-04  1.57e-05  1.16e-04  2.35e-07  0.542  0.0150
    v1-352x2-nc3  fused           44   |    2.04e-03  1.30e-04  4.69e-04  3.87e-06  0.230  0.0297 |    3.43e-04  3.36e-06  3.49e-05  3.61e-08  0.102  0.0107
    v1-352x2-nc3  fused           22   |    1.90e-03  1.26e-04  9.10e-04  5.90e-06  0.478  0.0469 |    1.17e-04  1.82e-06  1.47e-05  3.52e-08  0.126  0.0193
    v1-352x2-nc3  fused           11   |    7.59e-04  7.48e-05  5.17e-05  9.87e-07  0.068  0.0132 |    1.08e-04  3.08e-06  1.20e-05  1.42e-07  0.111  0.0461
    v1-352x2-nc3  three_launch    44   |    2.47e-03  1.95e-04  9.95e-04  5.07e-06  0.403  0.0260 |    3.41e-04  1.28e-05  1.61e-04  4.80e-08  0.471  0.0038
    v1-352x2-nc3  three_launch    22   |    2.66e-03  1.86e-04  1.18e-03  9.55e-06  0.444  0.0515 |    9.72e-05  8.31e-06  1.12e-08  8.90e-10  0.000  0.0001
    v1-352x2-nc3  three_launch    11   |    9.12e-04  1.54e-04  3.10e-04  2.22e-06  0.341  0.0144 |    1.54e-04  1.29e-05  1.15e-08  1.71e-09  0.000  0.0001
    v2-320x5-nc1  fused           40   |    3.03e-03  1.49e-04  7.27e-04  4.91e-06  0.240  0.0330 |    1.19e-04  5.54e-06  2.24e-05  9.04e-08  0.189  0.0163
    v2-320x5-nc1  fused           20   |    1.67e-03  9.82e-05  1.16e-03  3.35e-06  0.696  0.0341 |    3.62e-04  2.71e-05  3.56e-04  6.28e-07  0.983  0.0232
    v2-320x5-nc1  fused           10   |    2.09e-03  1.24e-04  6.97e-04  7.94e-06  0.333  0.0641 |    6.75e-05  9.97e-06  1.20e-05  2.46e-07  0.178  0.0247
    v2-320x5-nc1  three_launch    40   |    3.15e-03  2.11e-04  1.75e-03  9.18e-06  0.555  0.0435 |    1.26e-04  1.53e-05  1.33e-04  8.68e-08  1.056  0.0057
    v2-320x5-nc1  three_launch    20   |    1.98e-03  1.72e-04  1.54e-03  5.50e-06  0.781  0.0320 |    3.44e-04  4.34e-05  4.00e-04  7.17e-07  1.163  0.0165
    v2-320x5-nc1  three_launch    10   |    2.68e-03  1.99e-04  9.27e-04  9.17e-06  0.346  0.0462 |    1.21e-04  2.79e-05  1.39e-08  3.83e-09  0.000  0.0001
    v2-352x2-nc3  fused           44   |    2.96e-03  1.56e-04  1.36e-03  5.12e-06  0.460  0.0329 |    2.95e-04  3.98e-06  3.70e-05  6.60e-08  0.125  0.0166
    v2-352x2-nc3  fused           22   |    1.95e-03  1.73e-04  1.07e-03  7.87e-06  0.553  0.0455 |    9.99e-05  3.10e-06  1.93e-05  6.07e-08  0.193  0.0196
    v2-352x2-nc3  fused           11   |    1.01e-03  1.38e-04  4.47e-04  3.79e-06  0.441  0.0274 |    2.95e-04  8.41e-06  2.98e-05  3.42e-07  0.101  0.0407
    v2-352x2-nc3  three_launch    44   |    3.12e-03  2.10e-04  1.18e-03  1.12e-05  0.379  0.0535 |    2.96e-04  1.01e-05  1.70e-04  7.44e-08  0.577  0.0074
    v2-352x2-nc3  three_launch    22   |    2.10e-03  2.21e-04  9.35e-04  8.69e-06  0.444  0.0394 |    1.52e-04  1.06e-05  5.57e-05  2.05e-08  0.368  0.0019
    v2-352x2-nc3  three_launch    11   |    1.10e-03  1.72e-04  6.29e-04  1.02e-05  0.572  0.0593 |    2.87e-04  1.65e-05  1.53e-04  2.60e-07  0.534  0.0158
    v1-352x2-nc3  A32             44   |    2.04e-03  1.30e-04  4.69e-04  3.37e-06  0.230  0.0259 |    3.43e-04  3.36e-06  3.49e-05  2.76e-08  0.102  0.0082
    v1-352x2-nc3  A32             22   |    1.90e-03  1.26e-04  9.10e-04  6.24e-06  0.478  0.0496 |    1.17e-04  1.82e-06  1.47e-05  3.58e-08  0.126  0.0197
    v1-352x2-nc3  A32             11   |    7.59e-04  7.48e-05  3.96e-05  9.51e-07  0.052  0.0127 |    1.08e-04  3.08e-06  7.91e-06  7.18e-08  0.073  0.0233
    v1-352x2-nc3  2WG             44   |    2.04e-03  1.30e-04  4.69e-04  3.37e-06  0.230  0.0259 |    3.43e-04  3.36e-06  3.49e-05  2.76e-08  0.102  0.0082
    v1-352x2-nc3  2WG             22   |    1.90e-03  1.26e-04  9.10e-04  6.24e-06  0.478  0.0496 |    1.17e-04  1.82e-06  1.47e-05  3.58e-08  0.126  0.0197
    v1-352x2-nc3  2WG             11   |    7.59e-04  7.48e-05  3.96e-05  9.51e-07  0.052  0.0127 |    1.08e-04  3.08e-06  7.91e-06  7.18e-08  0.073  0.0233
    v1-352x2-nc3  1WG             44   |    2.04e-03  1.30e-04  4.69e-04  3.37e-06  0.230  0.0259 |    3.43e-04  3.36e-06  3.49e-05  2.76e-08  0.102  0.0082
    v1-352x2-nc3  1WG             22   |    1.90e-03  1.26e-04  9.10e-04  6.24e-06  0.478  0.0496 |    1.17e-04  1.82e-06  1.47e-05  3.58e-08  0.126  0.0197
    v1-352x2-nc3  1WG             11   |    7.59e-04  7.48e-05  3.96e-05  9.51e-07  0.052  0.0127 |    1.08e-04  3.08e-06  7.91e-06  7.18e-08  0.073  0.0233
    v2-352x2-nc3  A32             44   |    2.96e-03  1.56e-04  1.36e-03  6.19e-06  0.460  0.0398 |    2.95e-04  3.98e-06  3.70e-05  6.48e-08  0.125  0.0163
    v2-352x2-nc3  A32             22   |    1.95e-03  1.73e-04  1.07e-03  4.88e-06  0.553  0.0282 |    9.99e-05  3.10e-06  1.93e-05  7.01e-08  0.193  0.0226
    v2-352x2-nc3  A32             11   |    1.01e-03  1.38e-04  4.70e-04  5.03e-06  0.464  0.0364 |    2.95e-04  8.41e-06  1.50e-05  2.40e-07  0.051  0.0285
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import head_ref as HR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF, PER_IMAGE = 0.25, 8
CASES = [(preset, size, batch, nc) for preset in ("v1", "v2") for size, batch, nc in ((320, 5, 1), (352, 2, 3))]
_BUILT = {}


def _ids(p):
    return f"{p[0]}-{p[1]}x{p[2]}-nc{p[3]}"


def _build(param, tmp_path_factory):
    """A seeded model whose class bias is calibrated to ~8 candidates per image from the engine's own out0 (as
    test_gpu_head_skip.py), its images and its heads; once per case, shared."""
    if param in _BUILT:
        return _BUILT[param]
    from litepi import Engine, ncnn_export
    from oracle import ncnn_ref
    preset, S, B, nc = param
    d = tmp_path_factory.mktemp(f"head64_{preset}_{S}_{nc}")
    p, b = str(d / "m.param"), str(d / "m.bin")
    ncnn_export.export_detector(p, b, preset, seed=6400 + S + nc, nc=nc, cls_bias=0.0, size=S)
    imgs = np.random.default_rng(11 * S + nc).integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    e = Engine(precision="fp16", max_batch=B, max_det=300, det_input=S)
    try:
        e.load_detector(p, b)
        s = np.sort(e.detect_raw(imgs)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    finally:
        e.close()
    k = PER_IMAGE * B
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(CONF / (1 - CONF)) - mid), nc=nc)
    heads = HR.find_heads(ncnn_ref.load_model(p, b))
    assert len(heads) == 3
    anchors, strides = ncnn_export.make_anchors(S)
    imgs_path = str(d / "imgs.npy")
    np.save(imgs_path, imgs)
    _BUILT[param] = dict(param=param, p=p, b=b, imgs=imgs, imgs_path=imgs_path, heads=heads, anchors=anchors, strides=strides, dir=d)
    return _BUILT[param]


@pytest.fixture(scope="module", params=CASES, ids=_ids)
def model(request, tmp_path_factory):
    return _build(request.param, tmp_path_factory)


def _run(m):
    """One fp16 engine on the case: out0 of detect_raw, the three neck maps of that call (every image), the launches' names."""
    from litepi import Engine
    from litepi._ffi import LitepiError
    _, S, B, _ = m["param"]
    e = Engine(precision="fp16", max_batch=B, max_det=300, det_input=S)
    try:
        e.load_detector(m["p"], m["b"])
        out0 = np.array(e.detect_raw(m["imgs"]))
        # a refusal here is a defect of Detector::fetch_blob: the head reads these maps from HBM
        maps = [e.debug_blob(h["feat"], batch=B) for h in m["heads"]]
        with pytest.raises(LitepiError):   # more images than the handle holds: refused, nothing is read
            e.debug_blob(m["heads"][0]["feat"], batch=B + 1)
        e.profile_next(True)
        e.detect_raw(m["imgs"])
        names = [k["name"] for k in e.profile_read()]
    finally:
        e.close()
    return out0, maps, names


def _check(m, out0, maps, three_launch, tag):
    _, S, B, nc = m["param"]
    assert out0.shape == (B, 4 + nc, m["anchors"].shape[1]) and np.isfinite(out0).all()
    dfl = np.arange(16, dtype=np.float64)
    failures, off = [], 0
    for h, feat in zip(m["heads"], maps):
        assert feat.shape[0] == B and feat.shape[2] * (S // feat.shape[2]) == S, feat.shape
        H, W = feat.shape[2:]
        assert np.isfinite(feat).all() and (feat == feat.astype(np.float16)).all(), f"{tag}: map {h['feat']} is not fp16-exact"
        assert feat.std() > 0.05, f"{tag}: map {h['feat']} looks unwritten"
        stride = float(m["strides"][off])
        args = (feat, h, m["anchors"][:, off:off + H * W], stride, dfl)
        exact = HR.head_out0(*args, round_mid=False, round_logits=False)
        emul = HR.head_out0(*args, round_mid=True, round_logits=three_launch)
        st = HR.measure(out0[:, :, off:off + H * W], exact, emul, stride)
        print(f"{tag} level {H}x{W}: {HR.fmt(st)}")
        for k, s in st.items():
            if s["max_e"] < HR.MIN_MAX_E[k]:
                failures.append(f"level {H} {k}: max e {s['max_e']:.2e} < {HR.MIN_MAX_E[k]}: the budget is vacuous")
        failures += [f"level {H} {f}" for f in HR.broken_caps(st, HR.MEAN_CAP)]
        off += H * W
    assert off == out0.shape[2]
    assert not failures, f"{tag}: " + " | ".join(failures)


@pytest.mark.parametrize("plan", ["fused", "three_launch"])
def test_head_equals_float64_reference_of_its_input(model, plan, monkeypatch):
    if plan == "three_launch":
        monkeypatch.setenv("LITEPI_NO_HEADFUSE", "1")   # read when the model is loaded
    else:
        monkeypatch.delenv("LITEPI_NO_HEADFUSE", raising=False)
    out0, maps, names = _run(model)
    assert any(n.startswith("head_fused<") for n in names) == (plan == "fused"), names
    assert ("decode_f16" in names) == (plan == "three_launch"), names
    _check(model, out0, maps, plan == "three_launch", f"{_ids(model['param'])} {plan}")


# A fresh process per kernel-shape switch (read per load): the engine's out0, maps and launch names of the parent's model -> .npz
_CHILD = r"""
import sys
import numpy as np
from litepi import Engine
p, b, imgs_path, out, S, B = sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6])
feats = sys.argv[7:]
imgs = np.load(imgs_path)
e = Engine(precision="fp16", max_batch=B, max_det=300, det_input=S)
try:
    e.load_detector(p, b)
    res = {"out0": np.array(e.detect_raw(imgs))}
    for i, f in enumerate(feats):
        res[f"map{i}"] = e.debug_blob(f, batch=B)
    e.profile_next(True)
    e.detect_raw(imgs)
    res["names"] = np.array([k["name"] for k in e.profile_read()])
finally:
    e.close()
np.savez(out, **res)
"""

# the P3 / P4 / P5 instantiations HeadLayer::launch reaches behind each switch (v1: one class row tile, Cin 32 / 64 / 128)
SWITCHES = {
    "LITEPI_HEAD_A32": ["head_fused<1,2,1,2,2,8>_f16", "head_fused<1,3,2,4,4,12>_f16", "head_fused<1,2,1,4,8,24>_f16"],
    "LITEPI_HEAD_2WG": ["head_fused<1,2,1,2,2,12>_f16", "head_fused<1,3,2,4,6,24>_f16", "head_fused<1,2,1,4,8,24>_f16"],
    "LITEPI_HEAD_1WG": ["head_fused<1,3,2,2,6,24>_f16", "head_fused<1,3,2,4,6,24>_f16", "head_fused<1,2,1,4,8,24>_f16"],
    # v2 (two class row tiles, Cin 48 / 96 / 192): the three rows of the table without 16-pixel tiles
    "v2:LITEPI_HEAD_A32": ["head_fused<2,3,2,3,3,24>_f16", "head_fused<2,2,1,3,6,24>_f16", "head_fused<2,1,1,5,6,24>_f16"],
}


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_switched_shapes_equal_float64_reference(tmp_path_factory, tmp_path, switch):
    names_want = SWITCHES[switch]
    preset, _, switch = switch.rpartition(":")
    m = _build((preset or "v1", 352, 2, 3), tmp_path_factory)
    _, S, B, _ = m["param"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("LITEPI_HEAD_") and k != "LITEPI_NO_HEADFUSE"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "yolo-litepi_amd"), ROOT, env.get("PYTHONPATH", "")])
    env[switch] = "1"
    out = tmp_path / "out.npz"
    r = subprocess.run([sys.executable, "-c", _CHILD, m["p"], m["b"], m["imgs_path"], str(out), str(S), str(B)] + [h["feat"] for h in m["heads"]],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out) as z:
        out0, maps, names = z["out0"], [z[f"map{i}"] for i in range(3)], [str(n) for n in z["names"]]
    assert sorted(n for n in names if n.startswith("head_fused<")) == sorted(names_want), names
    _check(m, out0, maps, False, f"{_ids(m['param'])} {switch}")
