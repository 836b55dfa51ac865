"""The detector's execution plans, pinned launch by launch against a recording.

The planner (csrc/detector_plan.cpp) allocates device buffers as it goes, so it cannot run without a GPU; what a load planned
shows in the per-launch profile.  For every case below one handle is built, the model loaded, ONE seeded random image run
through detect_raw with profile_next(True), and the list of (kernel name, layer string, flops, bytes) of profile_read()
compared with tests/golden/detector_plans.json: names and layers exactly, flops and bytes to a relative 1e-9 (room for a
re-associated sum of doubles, not for another formula).  For the same handle every blob name of the .param is asked of
debug_blob, and which of them are handed out, refused as "fused away (never stored)", refused as living inside a whole-C2f
launch, or unknown to the plan (a Swish's input, the Detect tail) is compared too: the planner's materialised / in_c2f flags.

No output values are recorded: they change with every kernel, the plan does not.

    python tests/test_gpu_plan_golden.py --record     # rewrites the JSON from the same case list (on the GPU)

The recording is made with the build BEFORE a change to the planner, never with the code under change.
"""
import json
import os
import sys
import tempfile

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_JSON = os.path.join(_ROOT, "tests", "golden", "detector_plans.json")
_REF = os.path.join(_ROOT, "oracle", "_ref")

# every switch a case sets; all of them are cleared before a case sets its own
SWITCHES = ("LITEPI_NO_C2F", "LITEPI_NO_S2C", "LITEPI_NO_STEMBLOCK", "LITEPI_NO_HEADFUSE", "LITEPI_HEADFUSE", "LITEPI_C2F_XCV1",
            "LITEPI_NO_C2F_XCV1", "LITEPI_C2F_SKIP", "LITEPI_C2F_STORE_ALL")
_SKIP_20x20 = "c2f<64,1,s2+256>;c2f<64,1,s2+128,sppf>"   # test_v1_split_20x20_modules_vs_layer_plan's value


def _case(model, prec, size, cap, impl=0, env=None, tag=None):
    cid = f"{model}-{prec}-{size}-cap{cap}" + ("-naive" if impl else "") + (f"-{tag}" if tag else "")
    return dict(id=cid, model=model, prec=prec, size=size, cap=cap, impl=impl, env=env or {})


CASES = [_case(m, "fp16", 640, 64) for m in ("v1", "v2")]            # the benchmarked plans
CASES += [_case(m, "fp16", 640, 2) for m in ("v1", "v2")]            # the layer plan (whole-C2f is off below 4 images)
CASES += [_case(m, "fp16", 320, 4) for m in ("v1", "v2")]            # mixed: some modules fall back
CASES += [_case("v1", "fp16", 800, 4)]                               # every module falls back
CASES += [_case("v2", "fp16", 416, 4)]                               # stem block on partial tiles, every module on the layer plan
CASES += [_case(m, "fp32", 640, 4) for m in ("v1", "v2")]            # un-fused head + the decode launch
CASES += [_case("v1", "fp32", 640, 2, impl=1)]                       # naive conv implementation
for _m in ("v1", "v2"):                                              # the switches the suite toggles inside a process
    CASES += [_case(_m, "fp16", 640, 4, env={"LITEPI_NO_C2F": "1", "LITEPI_NO_S2C": "1"}, tag="no_c2f_no_s2c"),
              _case(_m, "fp16", 640, 4, env={"LITEPI_NO_STEMBLOCK": "1"}, tag="no_stemblock"),
              _case(_m, "fp16", 640, 4, env={"LITEPI_NO_HEADFUSE": "1"}, tag="no_headfuse")]
    CASES += [_case(_m, "fp16", 640, 4, env={"LITEPI_HEADFUSE": "narrow"}, tag="headfuse_narrow")] if _m == "v2" else []
    CASES += [_case(_m, "fp16", 640, 4, env={"LITEPI_C2F_XCV1": "1"}, tag="c2f_xcv1")] if _m == "v1" else []
    CASES += [_case(_m, "fp16", 640, 4, env={"LITEPI_NO_C2F_XCV1": "1"}, tag="no_c2f_xcv1")] if _m == "v2" else []
    CASES += [_case(_m, "fp16", 640, 4, env={"LITEPI_C2F_SKIP": _SKIP_20x20}, tag="c2f_skip")]
CASES += [_case(f, p, 640, 4) for f in ("yolo8", "yolo5", "yolo11") for p in ("fp16", "fp32")]   # the reference's baseline graphs
_IDS = [c["id"] for c in CASES]
assert len(set(_IDS)) == len(_IDS)


def _param_blobs(param):
    """Every blob name of an NCNN .param, in file order."""
    names, seen = [], set()
    with open(param) as f:
        lines = f.read().splitlines()[2:]
    for ln in lines:
        t = ln.split()
        if len(t) < 4:
            continue
        nin, nout = int(t[2]), int(t[3])
        for b in t[4:4 + nin + nout]:
            if b not in seen:
                seen.add(b)
                names.append(b)
    return names


def _model_files(case, workdir):
    """(param, bin) of a case, or None when the reference's graph files are not staged.  Seeded weights throughout."""
    from litepi import ncnn_export
    if case["model"] in ("v1", "v2"):
        param = os.path.join(workdir, f"{case['model']}_{case['size']}.param")
        binf = param[:-6] + ".bin"
        if not os.path.exists(param):
            ncnn_export.export_detector(param, binf, case["model"], seed=77, cls_bias=-2.0, size=case["size"])
        return param, binf
    param = os.path.join(_REF, f"{case['model']}_tt100k.param")
    if not os.path.exists(param):
        return None
    binf = os.path.join(workdir, f"{case['model']}.bin")
    if not os.path.exists(binf):
        ncnn_export.seeded_bin_for_param(param, binf, seed=5)
    return param, binf


def _blob_outcome(e, name):
    from litepi._ffi import LitepiError
    try:
        e.debug_blob(name)
        return "ok"
    except LitepiError as err:
        msg = str(err)
        if "lives inside a whole-C2f launch" in msg:
            return "in_c2f"
        if "fused away (never stored)" in msg:
            return "never_stored"
        if "unknown blob" in msg:
            return "unknown"
        return msg   # nothing else is expected: a recording or a comparison shows it in full


def observe(case, param, binf):
    """What the plan of one case looks like from outside: its launches and what debug_blob does with every blob."""
    from litepi import Engine
    img = np.random.default_rng(7).integers(0, 256, (1, case["size"], case["size"], 3), dtype=np.uint8)
    e = Engine(precision=case["prec"], max_batch=case["cap"], det_input=case["size"], conv_impl=case["impl"])
    try:
        e.load_detector(param, binf)
        e.profile_next(True)
        e.detect_raw(img)
        launches = [[k["name"], k["layer"], k["flops"], k["bytes"]] for k in e.profile_read()]
        blobs = {}
        for b in _param_blobs(param):
            blobs.setdefault(_blob_outcome(e, b), []).append(b)
    finally:
        e.close()
    return dict(launches=launches, blobs=blobs)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("plan_models"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_plan_matches_recording(case, golden, workdir, monkeypatch):
    files = _model_files(case, workdir)
    if files is None:
        pytest.skip("reference graph files not staged under oracle/_ref (__graft_entry__.build() stages them)")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    got = observe(case, *files)
    exp = golden[case["id"]]
    print(f"{case['id']}: {len(got['launches'])} launches; blobs " + ", ".join(f"{k} {len(v)}" for k, v in sorted(got["blobs"].items())))
    assert [(l[0], l[1]) for l in got["launches"]] == [(l[0], l[1]) for l in exp["launches"]]
    for g, x in zip(got["launches"], exp["launches"]):
        for q, what in ((2, "flops"), (3, "bytes")):
            assert abs(g[q] - x[q]) <= 1e-9 * abs(x[q]), f"{g[0]} ({g[1]}): {what} {g[q]!r}, recorded {x[q]!r}"
    assert got["blobs"] == exp["blobs"]


def record():
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "yolo-litepi_amd")]
    out = {}
    with tempfile.TemporaryDirectory(prefix="litepi_plans_") as workdir:
        for case in CASES:
            files = _model_files(case, workdir)
            if files is None:
                raise SystemExit(f"{case['id']}: {_REF} is not staged; a recording holds every case")
            for k in SWITCHES:
                os.environ.pop(k, None)
            os.environ.update(case["env"])
            out[case["id"]] = observe(case, *files)
            print(f"{case['id']}: {len(out[case['id']]['launches'])} launches", flush=True)
    with open(GOLDEN_JSON, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items()) + "\n}\n")
    print(f"wrote {GOLDEN_JSON} ({os.path.getsize(GOLDEN_JSON)} bytes)")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        raise SystemExit(__doc__)
    record()
