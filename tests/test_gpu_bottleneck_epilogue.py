"""GPU tests that pin the output of the fused bottleneck kernel (bottleneck_mfma_kernel, conv_kernels.hip: the ``bottleneck3x3x2<..>``
launches) bit for bit across a rewrite of its epilogues' addressing and predicates.  The arithmetic, the rounding points and the
MFMA operands of that kernel are not allowed to move, so ``detect_raw`` must stay byte-equal to what the kernel gave before.

Cases: seeded detectors (``ncnn_export.export_detector(preset, seed=77, cls_bias=-2.0, size=..)``), v1 and v2, fp16, at input sizes
whose stride-4 and stride-8 maps (the 160 x 160 and 80 x 80 levels of a 640 input) hold, under the planner's tile rule
(cplan::plan_bneck: tiles 20x40, 16x40, 10x20, 8x40, 8x20, 4x20):
    160 x 160   maps 40 x 40 / 20 x 20: whole tiles only (2 x 1 of 20x40, 2 x 1 of 10x20)
    160 x 352   maps 40 x 88 / 20 x 44: tiles cut on the right, whole at the bottom
    352 x 160   maps 88 x 40 / 44 x 20: whole on the right; the 80-level cv2 launch (10x20 / 8x20 tiles) cut at the bottom
    352 x 352   maps 88 x 88 / 44 x 44: cut on both sides
    416 x 416   maps 104 x 104 / 52 x 52: cut on both sides, other tiles (16x40 at batch 1)
     96 x  96   maps 24 x 24 / 12 x 12: one tile larger than the map
each with handles of capacity 1 and 5 (all images given): the layer plan of small handles and the whole-C2f plan of larger ones both
reach the kernel, with different tiles.  One fp32 case (v1, 96 x 96, batch 1) pins the SG == 0 path (gathered K steps as a loop).

Every case asserts that its profile (``profile_read``) holds ``bottleneck3x3x2<`` launches, and that out0 equals the recording in
tests/golden/bottleneck_epilogue.npz: the SHA-256 of the whole float32 array [B, 4 + nc, A] (bit for bit), and, so that a
mismatch can be located, the values of every k-th anchor (at most 300 per case) compared exactly first.

The recording was made on an MI355X with the library built from the commit BEFORE the epilogue rewrite:
    python tests/test_gpu_bottleneck_epilogue.py --record
runs the same cases and writes the file (it refuses to overwrite one that exists).  Re-record only when a change is MEANT to move
the kernel's results, and say so.
"""
import hashlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bottleneck_epilogue.npz")
SIZES = [(160, 160), (160, 352), (352, 160), (352, 352), (416, 416), (96, 96)]
CASES = [(preset, "fp16", size, batch) for preset in ("v1", "v2") for size in SIZES for batch in (1, 5)] + [("v1", "fp32", (96, 96), 1)]
SAMPLE = 300   # anchors kept verbatim per case


def _key(case):
    preset, prec, (h, w), batch = case
    return f"{preset}_{prec}_{h}x{w}_b{batch}"


def _run(case, workdir):
    """out0 of the case and the names of the launches of one profiled call."""
    from litepi import Engine, ncnn_export
    preset, prec, size, batch = case
    p, b = os.path.join(workdir, "m.param"), os.path.join(workdir, "m.bin")
    ncnn_export.export_detector(p, b, preset, seed=77, cls_bias=-2.0, size=size)
    imgs = np.random.default_rng(1000 * size[0] + size[1] + batch).integers(0, 256, (batch, size[0], size[1], 3), dtype=np.uint8)
    e = Engine(precision=prec, max_batch=batch, det_input=size)
    try:
        e.load_detector(p, b)
        out0 = e.detect_raw(imgs)
        e.profile_next(True)
        again = e.detect_raw(imgs)
        names = [k["name"] for k in e.profile_read()]
    finally:
        e.close()
    assert out0.tobytes() == again.tobytes(), "two calls on the same handle differ"
    return out0, names


def _digest(out0):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(out0, dtype=np.float32).tobytes()).digest(), dtype=np.uint8)


def _sample(out0):
    step = -(-out0.shape[2] // SAMPLE)
    return np.ascontiguousarray(out0[:, :, ::step])


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_out0_equals_recording(case, golden, tmp_path):
    out0, names = _run(case, str(tmp_path))
    bneck = sorted({n for n in names if n.startswith("bottleneck3x3x2<")})
    print(f"{_key(case)}: out0 {out0.shape}, {len(names)} launches, bottleneck launches: {bneck}")
    assert bneck, f"no bottleneck3x3x2 launch in the profile: {sorted(set(names))}"
    assert np.isfinite(out0).all()
    key = _key(case)
    want = golden[key + "/sample"]
    got = _sample(out0)
    assert got.shape == want.shape
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (f"{int(diff.sum())} of {diff.size} sampled values differ from the recording; first at "
                            f"(image, row, sampled anchor) {tuple(int(v) for v in np.argwhere(diff)[0])}, "
                            f"largest difference {float(np.abs(got - want).max()):.3e}")
    assert bytes(_digest(out0)) == bytes(golden[key + "/sha256"]), "sampled anchors equal the recording, the whole out0 does not"


def _record():
    import tempfile
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "yolo-litepi_amd"))
    out = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    if os.path.exists(out):
        raise SystemExit(f"{out} exists: remove it first if the kernel's results are meant to change")
    rec = {}
    for case in CASES:
        with tempfile.TemporaryDirectory() as d:
            out0, names = _run(case, d)
        bneck = sorted({n for n in names if n.startswith("bottleneck3x3x2<")})
        assert bneck, (case, sorted(set(names)))
        rec[_key(case) + "/sample"] = _sample(out0)
        rec[_key(case) + "/sha256"] = _digest(out0)
        print(f"{_key(case)}: out0 {out0.shape}, bottleneck launches {bneck}", flush=True)
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--record":
        _record()
    else:
        raise SystemExit("usage: python tests/test_gpu_bottleneck_epilogue.py --record [FILE]")
