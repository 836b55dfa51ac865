"""The launch lists of the frame fronts (lp_run_batch*, lp_run_tiled*, lp_run_views*, lp_run_focus*, lp_run_surfaces_device,
lp_run_views_surfaces_device), pinned against a recording.

The families share their host side (csrc/pipeline.cpp: one staged host pass and one device pass; csrc/views.cpp: one view
layout, one gather, one front), so a change there must leave what every entry point enqueues alone.  For every case below the call is made once with
profile_next(True) -- device paths followed by synchronize() -- and the list of (kernel name, layer string, flops, bytes) of
profile_read() is compared with tests/golden/front_launches.json: names and layers exactly, flops and bytes to a relative
1e-9.  The byte counts of the gather records (letterbox_u8, tile_crop_u8, window_views_u8) are computed on the host from the
layout, and those of the ROI stage and the classifier scale with the number of ROIs the call found, so the recording also
holds the layout's view counts and the detector's result indirectly.

Models are test_gpu_views.make_models (seeded, det_input 320); the engine is fp16 with max_batch 16.  The two frames are cut
from synth.config4_images: 300 x 310 (one view under tiling) and 400 x 500 (2 x 2 crops at overlap 64).  The tiled and views
cases must leave at least one record, so the ROI and classifier launches are part of their lists.  The focus cases create a
tracker and a default focus plan for their one call and destroy them again, so every other case runs on a handle without a
tracker; the surfaces cases take their planes from the NV12 conversion of the same frames (P010: every byte widened to
``byte << 8``).

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
# behind the cases above, so that those run before a handle has seen a tracker: focus views, and decoder surfaces
_CALLS_FOCUS = [
    ("run_focus", "run_focus", "mixed", {}, True),
    ("run_focus_device", "run_focus_device", "big", {}, True),
]
_CALLS_SURFACES = [
    ("run_surfaces_device", "run_surfaces_device", "big", {}, False, ("nv12", "p010")),
    ("run_views_surfaces_device-list", "run_views_surfaces_device", "big", dict(views=VIEW_LIST), True, ("nv12",)),
]
CASES = [dict(id=f"{stem}-{fmt}", method=m, frames=fr, kw=kw, finds=finds, fmt=fmt)
         for stem, m, fr, kw, finds in _CALLS + _CALLS_FOCUS for fmt in ("bgr", "nv12")]
CASES += [dict(id=f"{stem}-{fmt}", method=m, frames=fr, kw=kw, finds=finds, fmt=fmt)
          for stem, m, fr, kw, finds, fmts in _CALLS_SURFACES for fmt in fmts]
_IDS = [c["id"] for c in CASES]
assert len(set(_IDS)) == len(_IDS)


def make_engine(models):
    from litepi import Engine
    from litepi.backend import random_shufflenet_state
    e = Engine(precision="fp16", max_batch=16, max_det=300, num_classes=91, det_input=S)
    e.load_detector(models["param"], models["bin"])
    e.load_classifier(random_shufflenet_state(91, seed=3))
    return e


def make_frames(d):
    """models and frames all cases share"""
    import pixfmt_ref as R
    from test_gpu_views import make_models
    models = make_models(d)
    f0, f1 = models["frames"]
    bgr = {"mixed": [np.ascontiguousarray(f0[:SMALL[0], :SMALL[1]]), np.ascontiguousarray(f1[:BIG[0], :BIG[1]])],
           "big": [np.ascontiguousarray(f0[200:200 + BIG[0], 300:300 + BIG[1]]), np.ascontiguousarray(f1[:BIG[0], :BIG[1]])]}
    frames = {"bgr": bgr, "nv12": {k: [R.bgr_to_nv12(f) for f in v] for k, v in bgr.items()}}
    return dict(models=models, frames=frames)


def make_setup(d):
    """models, frames and the engine all cases share"""
    s = make_frames(d)
    s["engine"] = make_engine(s["models"])
    return s


def _surface(nv12, fmt):
    """tight NV12 frame [H * 3 // 2, W] -> (Surface, the device tensors that keep it alive)"""
    import torch
    from litepi.surfaces import surface_from_tensors
    f = (nv12.astype(np.uint16) << 8).view(np.int16) if fmt == "p010" else nv12
    H = f.shape[0] // 3 * 2
    planes = (torch.from_numpy(np.ascontiguousarray(f[:H])).cuda(), torch.from_numpy(np.ascontiguousarray(f[H:])).cuda())
    s, got = surface_from_tensors(*planes)
    assert got == fmt
    return s, planes


class Call:
    """One case's call on engine e: call() makes it (device paths followed by synchronize()) and returns the records found.
    like: a Call whose device frames or surfaces, and record and count buffers, this one uses too."""

    def __init__(self, e, frames, case, like=None):
        import torch
        self.e, self.m, self.kw, self.fmt = e, case["method"], case["kw"], case["fmt"]
        self.surf = "surfaces" in self.m
        self.frames = frames["nv12" if self.surf else self.fmt][case["frames"]]
        self.B = B = len(self.frames)
        if not self.m.endswith("_device"):
            return
        if like is not None and hasattr(like, "dd"):
            self.dd, self.dc = like.dd, like.dc
        else:
            self.dd = torch.zeros(B * e.cfg.max_det * 32, dtype=torch.uint8, device="cuda")
            self.dc = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        if self.surf:
            shared = like is not None and hasattr(like, "src") and like.surf and like.fmt == self.fmt
            self.src = like.src if shared else [_surface(f, self.fmt) for f in self.frames]
        else:
            shared = like is not None and hasattr(like, "src") and not like.surf and like.fmt == self.fmt
            self.src = like.src if shared else torch.from_numpy(np.stack(self.frames)).cuda()
        torch.cuda.synchronize()

    def __call__(self):
        e, m, kw, frames = self.e, self.m, self.kw, self.frames
        e.set_input_format("bgr" if self.surf else self.fmt)
        if not m.endswith("_device"):
            if m == "run_views":
                out = e.run_views(frames, kw["views"], CONF, IOU, MIN_AREA)
            else:
                out = getattr(e, m)(frames, CONF, IOU, MIN_AREA, **kw)
            return int(out[1].sum())
        tail = (CONF, IOU, MIN_AREA, self.dd.data_ptr(), self.dc.data_ptr())
        if self.surf:
            surfaces = [s for s, _ in self.src]
            if m == "run_surfaces_device":
                e.run_surfaces_device(surfaces, *tail, pixfmt=self.fmt)
            else:
                e.run_views_surfaces_device(surfaces, kw["views"], *tail, pixfmt=self.fmt)
        else:
            H, W = self.frames[0].shape[0] * (2 if self.fmt == "nv12" else 3) // 3, self.frames[0].shape[1]
            head = (self.src.data_ptr(), self.B, H, W)
            if m == "run_views_device":
                e.run_views_device(*head, kw["views"], *tail)
            else:   # run_batch_device, run_tiled_device, run_focus_device
                getattr(e, m)(*head, *tail, **kw)
        e.synchronize()
        return int(self.dc.cpu().numpy()[:self.B].sum())


def observe(setup, case):
    """(launches, records found) of one profiled call"""
    e = setup["engine"]
    call = Call(e, setup["frames"], case)
    focus = case["method"].startswith("run_focus")
    if focus:
        e.tracker_create()
        e.focus_create()
    try:
        e.profile_next(True)
        found = call()
        launches = [[k["name"], k["layer"], k["flops"], k["bytes"]] for k in e.profile_read()]
    finally:
        if focus:
            e.tracker_destroy()
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
