"""The launch lists of the frame fronts (lp_run_batch*, lp_run_tiled*, lp_run_views*), pinned against a recording.

The three families share their host side (csrc/views.cpp: one view layout, one gather, one staged host front and one device
front), so a change there must leave what every entry point enqueues alone.  For every case below the call is made once with
profile_next(True) -- device paths followed by synchronize() -- and the list of (kernel name, layer string, flops, bytes) of
profile_read() is compared with tests/golden/front_launches.json: names and layers exactly, flops and bytes to a relative
1e-9.  The byte counts of the gather records (letterbox_u8, tile_crop_u8, window_views_u8) are computed on the host from the
layout, and those of the ROI stage and the classifier scale with the number of ROIs the call found, so the recording also
holds the layout's view counts and the detector's result indirectly.

Models are test_gpu_views.make_models (seeded, det_input 320); the engine is fp16 with max_batch 16.  The two frames are cut
from synth.config4_images: 300 x 310 (one view under tiling) and 400 x 500 (2 x 2 crops at overlap 64).  The tiled and views
cases must leave at least one record, so the ROI and classifier launches are part of their lists.

    python tests/test_gpu_front_launches.py --record     # rewrites the JSON from the same case list (on the GPU)

The recording is made with the build BEFORE a change to the fronts, never with the code under change.
"""
import json
import os
import pathlib
import sys
import tempfile

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_JSON = os.path.join(_ROOT, "tests", "golden", "front_launches.json")

S = 320
CONF, IOU, MIN_AREA = 0.25, 0.45, 50
OVERLAP = 64
SMALL, BIG = (300, 310), (400, 500)   # H, W
# up-scales of 1.25, 2 and 8 at det_input 320 ...
VIEW_LIST = ["full", (3, 5, 256, 200), (101, 57, 160, 160), (20, 10, 40, 40)]
# ... and, beyond them, a down-scale (the frame as a window), the copy branch (w = h = det_input) and an up-scale in one list
SCALE_LIST = ["full", (0, 0, 500, 400), (13, 5, 320, 320), (101, 57, 160, 160)]

# (id stem, method, frames: "mixed" = SMALL + BIG / "big" = two BIG, extra arguments, must find something)
_CALLS = [
    ("run_batch", "run_batch", "mixed", {}, False),
    ("run_batch_device", "run_batch_device", "big", {}, False),
    ("run_tiled-full1", "run_tiled", "mixed", dict(overlap=OVERLAP, full_frame=True), True),
    ("run_tiled-full0", "run_tiled", "mixed", dict(overlap=OVERLAP, full_frame=False), True),
    ("run_tiled_device", "run_tiled_device", "big", dict(overlap=OVERLAP, full_frame=True), True),
    ("run_views-full", "run_views", "mixed", dict(views=["full"]), True),
    ("run_views-list", "run_views", "big", dict(views=VIEW_LIST), True),
    ("run_views_device-list", "run_views_device", "big", dict(views=VIEW_LIST), True),
    ("run_views-scales", "run_views", "big", dict(views=SCALE_LIST), True),
    ("run_views_device-scales", "run_views_device", "big", dict(views=SCALE_LIST), True),
]
CASES = [dict(id=f"{stem}-{fmt}", method=m, frames=fr, kw=kw, finds=finds, fmt=fmt)
         for stem, m, fr, kw, finds in _CALLS for fmt in ("bgr", "nv12")]
_IDS = [c["id"] for c in CASES]
assert len(set(_IDS)) == len(_IDS)


def make_setup(d):
    """models, frames and the engine all cases share"""
    import pixfmt_ref as R
    from litepi import Engine
    from litepi.backend import random_shufflenet_state
    from test_gpu_views import make_models
    models = make_models(d)
    f0, f1 = models["frames"]
    bgr = {"mixed": [np.ascontiguousarray(f0[:SMALL[0], :SMALL[1]]), np.ascontiguousarray(f1[:BIG[0], :BIG[1]])],
           "big": [np.ascontiguousarray(f0[200:200 + BIG[0], 300:300 + BIG[1]]), np.ascontiguousarray(f1[:BIG[0], :BIG[1]])]}
    frames = {"bgr": bgr, "nv12": {k: [R.bgr_to_nv12(f) for f in v] for k, v in bgr.items()}}
    e = Engine(precision="fp16", max_batch=16, max_det=300, num_classes=91, det_input=S)
    e.load_detector(models["param"], models["bin"])
    e.load_classifier(random_shufflenet_state(91, seed=3))
    return dict(engine=e, frames=frames)


def observe(setup, case):
    """(launches, records found) of one profiled call"""
    import torch
    e, frames, kw = setup["engine"], setup["frames"][case["fmt"]][case["frames"]], case["kw"]
    B = len(frames)
    e.set_input_format(case["fmt"])
    if case["method"].endswith("_device"):
        H, W = BIG
        dev = torch.from_numpy(np.stack(frames)).cuda()
        dd = torch.zeros(B * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
        dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        tail = (CONF, IOU, MIN_AREA, dd.data_ptr(), dc.data_ptr())
        e.profile_next(True)
        if case["method"] == "run_batch_device":
            e.run_batch_device(dev.data_ptr(), B, H, W, *tail)
        elif case["method"] == "run_tiled_device":
            e.run_tiled_device(dev.data_ptr(), B, H, W, *tail, **kw)
        else:
            e.run_views_device(dev.data_ptr(), B, H, W, kw["views"], *tail)
        e.synchronize()
        found = int(dc.cpu().numpy()[:B].sum())
    else:
        e.profile_next(True)
        if case["method"] == "run_views":
            out = e.run_views(frames, kw["views"], CONF, IOU, MIN_AREA)
        else:
            out = getattr(e, case["method"])(frames, CONF, IOU, MIN_AREA, **kw)
        found = int(out[1].sum())
    launches = [[k["name"], k["layer"], k["flops"], k["bytes"]] for k in e.profile_read()]
    return launches, found


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_JSON) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    s = make_setup(tmp_path_factory.mktemp("front_launches"))
    yield s
    s["engine"].close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_front_launches_match_recording(case, golden, setup):
    got, found = observe(setup, case)
    exp = golden[case["id"]]
    print(f"{case['id']}: {len(got)} launches, {found} records; gather " +
          ", ".join(f"{l[0]} {l[3]:.0f} B" for l in got if l[0] in ("letterbox_u8", "tile_crop_u8", "window_views_u8")))
    if case["finds"]:
        assert found >= 1, "the calibrated model found nothing: the ROI and classifier launches are missing from the list"
        assert any(l[0] == "roi_resize_pil" for l in got)
    assert [(l[0], l[1]) for l in got] == [(l[0], l[1]) for l in exp]
    for g, x in zip(got, exp):
        for q, what in ((2, "flops"), (3, "bytes")):
            assert abs(g[q] - x[q]) <= 1e-9 * abs(x[q]), f"{g[0]} ({g[1]}): {what} {g[q]!r}, recorded {x[q]!r}"


def record():
    sys.path[:0] = [_ROOT, os.path.join(_ROOT, "yolo-litepi_amd"), os.path.join(_ROOT, "tests")]
    out = {}
    with tempfile.TemporaryDirectory(prefix="litepi_fronts_") as workdir:
        setup = make_setup(pathlib.Path(workdir))
        try:
            for case in CASES:
                launches, found = observe(setup, case)
                if case["finds"] and found < 1:
                    raise SystemExit(f"{case['id']}: the calibrated model found nothing; a recording holds the ROI and classifier launches")
                out[case["id"]] = launches
                print(f"{case['id']}: {len(launches)} launches, {found} records", flush=True)
        finally:
            setup["engine"].close()
    with open(GOLDEN_JSON, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items()) + "\n}\n")
    print(f"wrote {GOLDEN_JSON} ({os.path.getsize(GOLDEN_JSON)} bytes)")


if __name__ == "__main__":
    if "--record" not in sys.argv:
        raise SystemExit(__doc__)
    record()
