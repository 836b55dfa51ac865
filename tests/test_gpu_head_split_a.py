"""GPU tests of the Detect head's split stage A (head_kernels.hip): on the default shapes a workgroup runs only the CLASS
tower's first 3x3 conv in front of its vote; the box tower's first conv -- two thirds of the merged stage A's rows -- runs behind
the vote, in the workgroups that stay, from an input tile that is staged a second time where ``MID`` overlays it.  Every output
channel still accumulates the same bias-initialised fp32 sum in the same K order, so nothing that the head emits may change by a
bit: the comparison side is the merged stage A of the same build (``LITEPI_HEAD_MERGED_A=1``), the tolerance is zero.

The switch is read per load; each side is a fresh child process, and children run one after another.

Shapes (both presets: the three default shapes of v1 and v2's P3 and P4 have the split stage A, v2's P5 keeps the merged one; v2's
P3 has an odd number of 16-channel groups per tap, so its zeroed guard slot behind the tile is staged again too): 320 x 320, batch 5 (whole-C2f plan; maps 40 / 20 / 10, a masked last tile
column at P3) and 352 x 352, batch 2 (layer plan; maps 44 / 22 / 11: masked edges both ways on every level), with one class and
with three.  ``detect_raw`` requests out0, so no workgroup leaves: the deferred box pass and the second staging of the tile run on
every tile, border tiles included."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFS = (0.25, 0.001, 0.999)


def _child_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LITEPI_HEAD_")}
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "yolo-litepi_amd"), ROOT, env.get("PYTHONPATH", "")])
    env.update(extra)
    return env


def _run_child(script, args, env):
    r = subprocess.run([sys.executable, "-c", script] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


# One side of the comparison: seeded weights and images, the class bias calibrated to ~8 candidates per image from the engine's own
# out0 (as test_gpu_head_skip.py), then out0 of detect_raw and the records and counts of detect at three thresholds -> one .npz.
_OUTPUT_SCRIPT = r"""
import sys
import numpy as np
from litepi import Engine, ncnn_export
work, S, B, nc, out, preset = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
p, b = work + "/m.param", work + "/m.bin"
ncnn_export.export_detector(p, b, preset, seed=4100 + S + nc, nc=nc, cls_bias=0.0, size=S)
imgs = np.random.default_rng(7 * S + nc).integers(0, 256, (B, S, S, 3), dtype=np.uint8)
e = Engine(precision="fp16", max_batch=B, max_det=300, det_input=S)
try:
    e.load_detector(p, b)
    s = np.sort(e.detect_raw(imgs)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
finally:
    e.close()
k = 8 * B
mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid), nc=nc)
e = Engine(precision="fp16", max_batch=B, max_det=2560, det_input=S)
res = {}
try:
    e.load_detector(p, b)
    res["out0"] = np.ascontiguousarray(e.detect_raw(imgs))
    for conf in (0.25, 0.001, 0.999):
        dets, counts = e.detect(list(imgs), conf, 0.45)
        counts = np.asarray(counts).astype(np.int64)
        res[f"counts_{conf}"] = counts
        res[f"records_{conf}"] = np.frombuffer(b"".join(np.ascontiguousarray(dets[i, :counts[i]]).tobytes() for i in range(B)), dtype=np.uint8)
finally:
    e.close()
np.savez(out, **res)
"""


@pytest.mark.parametrize("nc", [1, 3], ids=lambda v: f"nc{v}")
@pytest.mark.parametrize("size,batch", [(320, 5), (352, 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("preset", ["v1", "v2"])
def test_split_equals_merged_byte_for_byte(tmp_path, preset, size, batch, nc):
    sides = {}
    for tag, extra in (("merged", {"LITEPI_HEAD_MERGED_A": "1"}), ("split", {})):
        d = tmp_path / tag
        d.mkdir()
        out = d / "out.npz"
        _run_child(_OUTPUT_SCRIPT, [d, size, batch, nc, out, preset], _child_env(**extra))
        with np.load(out) as z:
            sides[tag] = {k: z[k] for k in z.files}
    m, s = sides["merged"], sides["split"]
    assert sorted(m) == sorted(s) and len(m) == 1 + 2 * len(CONFS)
    kept = {c: int(s[f"counts_{c}"].sum()) for c in CONFS}
    print(f"{preset} {size}x{size} batch {batch} nc {nc}: kept boxes {kept}, out0 {s['out0'].shape}")
    for k in sorted(m):
        a, b = np.ascontiguousarray(m[k]), np.ascontiguousarray(s[k])
        assert a.shape == b.shape and a.dtype == b.dtype, k
        differing = int((a.view(np.uint8) != b.view(np.uint8)).sum())
        print(f"  {k}: {a.nbytes} bytes, {differing} differ")
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{k}: split stage A differs from the merged one"
    assert np.isfinite(s["out0"]).all()
    assert kept[0.25] >= 1, "the calibrated case keeps no box: the comparison would be vacuous"
    assert kept[0.999] == 0, "conf 0.999 must keep nothing"
    assert kept[0.001] > kept[0.25]


# LITEPI_HEAD_STAMPS makes every head launch append a record [magic, grid, H, N][grid][16]: stamp 14 is 1 for a workgroup that left at
# the vote, stamps 10-13 are the start and the end of the box pass of the split stage A and of its SiLU epilogue.
_STAMP_SCRIPT = r"""
import json, os, sys
import numpy as np
from litepi import Engine, ncnn_export
work, S, B = sys.argv[1], 320, 5
stamps = os.environ["LITEPI_HEAD_STAMPS"]
p, b = os.path.join(work, "m.param"), os.path.join(work, "m.bin")
ncnn_export.export_detector(p, b, "v1", seed=11, cls_bias=0.0, size=S)
imgs = np.random.default_rng(5).integers(0, 256, (B, S, S, 3), dtype=np.uint8)
e = Engine(precision="fp16", max_batch=B, max_det=2560, det_input=S)
e.load_detector(p, b)
s = np.sort(e.detect_raw(imgs)[:, 4].astype(np.float64).ravel())[::-1]
e.close()
k = 8 * B
mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - mid))
e = Engine(precision="fp16", max_batch=B, max_det=2560, det_input=S)
e.load_detector(p, b)
open(stamps, "wb").close()

def levels():
    raw = np.fromfile(stamps, dtype=np.uint64)
    open(stamps, "wb").close()
    out, off = [], 0
    while off < len(raw):
        assert raw[off] == 0x48454144
        grid, H = int(raw[off + 1]), int(raw[off + 2])
        st = raw[off + 4: off + 4 + grid * 16].reshape(grid, 16)
        left = st[:, 14] == 1
        box = st[:, 10:14]
        out.append({"H": H, "grid": grid, "left": int(left.sum()),
                    "leavers_with_box_stamps": int((box[left] != 0).any(axis=1).sum()),
                    "stayers_with_all_box_stamps": int((box[~left] != 0).all(axis=1).sum())})
        off += 4 + grid * 16
    return out

e.detect_raw(imgs)
res = {"raw": levels()}
_, counts = e.detect(list(imgs), 0.25, 0.45)
res["detect"] = levels()
res["kept"] = int(np.asarray(counts).sum())
e.close()
print("RESULT " + json.dumps(res))
"""


def test_box_pass_is_skipped_by_the_workgroups_that_leave(tmp_path):
    out = _run_child(_STAMP_SCRIPT, [tmp_path], _child_env(LITEPI_HEAD_STAMPS=str(tmp_path / "stamps.bin"), LITEPI_NO_GRAPH="1"))
    res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(res)
    assert [lv["H"] for lv in res["raw"]] == [40, 20, 10] and [lv["H"] for lv in res["detect"]] == [40, 20, 10]
    for lv in res["raw"]:   # out0 requested: nobody leaves, the box pass runs in every workgroup
        assert lv["left"] == 0 and lv["stayers_with_all_box_stamps"] == lv["grid"], lv
    for lv in res["detect"]:
        assert lv["leavers_with_box_stamps"] == 0, lv                                 # a leaver never reaches the box pass
        assert lv["stayers_with_all_box_stamps"] == lv["grid"] - lv["left"], lv       # a stayer runs all of it
    assert sum(lv["left"] for lv in res["detect"]) >= 1 and sum(lv["grid"] - lv["left"] for lv in res["detect"]) >= 1, "both kinds must occur"
    assert res["kept"] >= 1
