"""The geometry, limits, plan choice and weight preparation of the ShuffleNetV2 classifier (csrc/cls_plan.h) without a device.

tests/native/cls_plan_replay.cpp includes the header alone, built with a plain g++ under -fsanitize=address,undefined, as a stand-alone
program.  It prints every case of tests/golden/cls_plans.json -- what fold / expand_pw / expand_dw / pack_fused_pw / pack_cls_stem,
the LDS-size functions, the launchers' class-count checks and load()'s choice of plan computed BEFORE they moved into the header (see
the file's "about") -- and every size, hash, flag and name must be the recorded one."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cls_plans.json")

PW_PAIRS = ((64, 24), (64, 64), (128, 128), (240, 256), (240, 240), (1024, 480))   # every (cout_p, cin_p) of the network
FC_CLASSES = (1, 2, 58, 91, 256, 560)


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("cls_plan") / "cls_plan_replay")
    src = os.path.join(ROOT, "tests", "native", "cls_plan_replay.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", inc, src,
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        k, v = ln.split(" = ")
        assert k not in out, k
        out[k] = v
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_cases_are_the_issue_s_list(golden):
    c = golden["cases"]
    assert "commit" in golden["about"] and os.path.getsize(GOLDEN) < 64 * 1024
    for cout, cin in PW_PAIRS:
        assert f"pack_fused_pw {cout} {cin} 0" in c
    for nc in FC_CLASSES:
        assert f"pack_fused_pw {(nc + 15) // 16 * 16} 1024 {nc}" in c
    assert "pack_cls_stem" in c and {"fold 3x3", "fold 1x1", "fold depthwise"} <= set(c)
    assert {"expand_pw single", "expand_dw single"} <= set(c)
    for s in (2, 3, 4):
        assert {f"expand_pw stage{s}.s1", f"expand_pw stage{s}.in", f"expand_dw stage{s}.in"} <= set(c)
    assert {f"lds_stage {b}" for b in (64, 128, 240)} <= set(c) and "lds_head 480 256" in c
    assert {f"plan {p} {i} {s}" for p in ("fp16", "fp32") for i in (0, 1) for s in (0, 1)} <= set(c)


def test_every_case_matches_the_recording(golden, replay):
    assert list(replay) == list(golden["cases"])
    for k, want in golden["cases"].items():
        assert replay[k] == want, f"{k}: {replay[k]}, recorded {want}"


def test_packed_sizes_follow_the_fragment_format(replay):
    """[cout_p / 16 tiles][ceil(cin_p / 32) steps][64 lanes][8 halfs]"""
    for cout, cin in PW_PAIRS + tuple(((nc + 15) // 16 * 16, 1024) for nc in FC_CLASSES):
        keys = [k for k in replay if k.startswith(f"pack_fused_pw {cout} {cin} ")]
        assert keys
        for k in keys:
            assert int(replay[k].split()[0]) == cout // 16 * ((cin + 31) // 32) * 64 * 8 * 2, k


def test_limits_on_both_sides(replay):
    """cls_back takes up to 560 classes, cls_head_fused up to 256 (the refusals tests/test_gpu_classifier.py provokes at 561 / 257)"""
    assert (replay["back_supports 560"], replay["back_supports 561"]) == ("1", "0")
    assert (replay["head_supports 480 256"], replay["head_supports 480 257"]) == ("1", "0")
    assert replay["back_supports 1"] == "1" and replay["head_supports 480 1"] == "1" and replay["head_supports 484 91"] == "0"
    assert int(replay["lds_head 480 256"]) <= 160 * 1024 and int(replay["lds_stage 240"]) <= 160 * 1024


def test_plan_choice_is_the_paths_of_the_device_tests(replay):
    """paths A..E of tests/test_gpu_classifier.py: (precision, conv_impl, LITEPI_CLS_LAYERWISE) -> plan"""
    assert replay["plan fp16 0 0"] == "TWO_LAUNCH" and replay["plan fp16 0 1"] == "STAGE_FUSED"
    for k in ("fp16 1 0", "fp16 1 1", "fp32 0 0", "fp32 0 1", "fp32 1 0", "fp32 1 1"):
        assert replay["plan " + k] == "LAYERWISE", k
