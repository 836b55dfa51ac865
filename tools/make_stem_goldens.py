#!/usr/bin/env python3
"""Record tests/golden/stem_block_out0.npz: what detect_raw returns on the commit this script is run on, for the cases of
tests/test_gpu_stem_block_bits.py (which imports CASES and run_case from here, so that recorder and test cannot drift apart).

    python tools/make_stem_goldens.py            (needs the device and a built library)

The golden is recorded on the commit BEFORE a change to stem_block_kernel / stem_block16_kernel that must leave every output
byte as it was; the test then pins the changed kernels to it.  Per case it holds the SHA-256 of out0's bytes, its shape, the
names of the first profiled launches and 64 sampled values (flat index and value) for a readable failure message: a few KB.
Weights and images are seeded as in test_gpu_parity.test_stem_block16_equals_unfused_plan_v2.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "stem_block_out0.npz")
# (name, preset, (rows, columns), batch)
#   352 x 352 x2: 88 = 2.75 x 32 columns, 11 x 8 rows: border and partial tiles
#   640 x 640 x1: interior and border forms of the stem loop
#   384 x 640 x1: lp_config::det_input_h
CASES = [(f"{preset}_{h}x{w}_b{b}", preset, (h, w), b)
         for preset in ("v1", "v2") for (h, w), b in (((352, 352), 2), ((640, 640), 1), ((384, 640), 1))]
NSAMPLE = 64


def run_case(preset, hw, batch, workdir):
    """-> (out0, names of the launches of one profiled detect_raw)"""
    from litepi import Engine, ncnn_export
    h, w = hw
    size = h if h == w else (h, w)
    param, binf = os.path.join(workdir, "d.param"), os.path.join(workdir, "d.bin")
    ncnn_export.export_detector(param, binf, preset, seed=5, cls_bias=-2.0, size=size)
    imgs = np.random.default_rng(h * 1000 + w).integers(0, 256, (batch, h, w, 3), dtype=np.uint8)
    e = Engine(precision="fp16", max_batch=batch, det_input=size)
    try:
        e.load_detector(param, binf)
        out0 = e.detect_raw(imgs)
        e.profile_next(True)
        again = e.detect_raw(imgs)
        names = [k["name"] for k in e.profile_read()]
    finally:
        e.close()
    assert np.array_equal(out0.view(np.uint8), again.view(np.uint8)), "two calls of one handle differ"
    return np.ascontiguousarray(out0), names


def digest(out0):
    return hashlib.sha256(out0.tobytes()).hexdigest()


def sample_index(size):
    return np.random.default_rng(size).choice(size, NSAMPLE, replace=False).astype(np.int64)


def main():
    for p in (ROOT, os.path.join(ROOT, "yolo-litepi_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    rec = {}
    for name, preset, hw, batch in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            out0, names = run_case(preset, hw, batch, tmp)
        idx = sample_index(out0.size)
        rec[name + "_sha256"] = np.array(digest(out0))
        rec[name + "_shape"] = np.array(out0.shape, np.int64)
        rec[name + "_dtype"] = np.array(str(out0.dtype))
        rec[name + "_first"] = np.array(names[0])
        rec[name + "_idx"] = idx
        rec[name + "_val"] = out0.ravel()[idx].copy()
        print(f"{name}: {out0.shape} {out0.dtype} first launch {names[0]} sha256 {digest(out0)[:16]}")
    np.savez_compressed(GOLDEN, **rec)
    print(f"wrote {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
