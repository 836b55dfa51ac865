"""GPU tests of the Detect head's early exit (head_kernels.hip): a workgroup runs the class tower and the class projection
of its tile first, votes on whether any anchor of the tile can pass ``conf``, and leaves in front of the box tower when none
can.  Neither tower's arithmetic changes, so the product path (``detect``: tiles may leave) must reproduce, record for
record, what the reference's postprocess makes of the SAME handle's non-skipping path (``detect_raw``: out0 is requested, no
workgroup leaves, every anchor is decoded).

Shapes: 320 x 320, batch 5 (capacity >= 4: the whole-C2f plan; maps 40 / 20 / 10: P3 has 5 x 3 tiles of 8 x 16 with a masked
last column, P4 2 x 1 tiles of 10 x 20, P5 one tile) and 352 x 352, batch 2 (layer plan; maps 44 / 22 / 11: masked edges in both
directions on every level), for both presets, with one class and with three (the vote must see the best of all classes).

Cases: calibrated to ~8 candidates per image (most tiles leave, some stay); conf 0.999 (every tile leaves) followed by 0.25 on
the same handle (no state survives a launch); conf 0.001 (no tile leaves); the device entry point three times on one handle
(eager, graph capture, graph replay)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CONF, IOU = 0.25, 0.45
PER_IMAGE = 8
MAX_DET = 2560


def _reference(out0, S, conf):
    from oracle import postprocess_ref as P
    return [P.postprocess(out0[i], (S, S), 1.0, (0.0, 0.0), conf, IOU) for i in range(len(out0))]


def _check_detect(eng, imgs, out0, conf, tag):
    """detect == postprocess(detect_raw): count, order, det_conf as floats, det_class, boxes after the int truncation.
    Returns the number of kept boxes per image."""
    S = imgs.shape[1]
    dets, counts = eng.detect(list(imgs), conf, IOU)
    kept = []
    for i, (eb, es, ec) in enumerate(_reference(out0, S, conf)):
        assert counts[i] == len(eb), f"{tag}: image {i}: {counts[i]} boxes vs {len(eb)}"
        for k in range(len(eb)):
            r = dets[i, k]
            got_box = tuple(int(r[f]) for f in ("x1", "y1", "x2", "y2"))
            assert got_box == tuple(int(v) for v in eb[k].astype(int)), f"{tag}: image {i} box {k}: {got_box} vs {eb[k]}"
            assert float(r["det_conf"]) == float(es[k]), f"{tag}: image {i} box {k}: score {r['det_conf']} vs {es[k]}"
            assert int(r["det_class"]) == int(ec[k]), f"{tag}: image {i} box {k}: class {r['det_class']} vs {ec[k]}"
        kept.append(len(eb))
    return kept


@pytest.fixture(scope="module", params=[(preset, size, batch, nc) for preset in ("v1", "v2") for size, batch in ((320, 5), (352, 2))
                                        for nc in (1, 3)], ids=lambda p: f"{p[0]}-{p[1]}x{p[2]}-nc{p[3]}")
def setup(request, tmp_path_factory):
    """One calibrated fp16 engine per (preset, shape, nc), its images and its own out0 (computed once, never modified)."""
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    preset, S, B, nc = request.param
    d = tmp_path_factory.mktemp(f"skip_{preset}_{S}_{nc}")
    p, b = str(d / "m.param"), str(d / "m.bin")
    ncnn_export.export_detector(p, b, preset, seed=2024 + S + nc, nc=nc, cls_bias=0.0, size=S)
    imgs = np.random.default_rng(S + nc).integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    # class bias from the k-th best score of the engine's own out0 (as bench.py:build_models), threshold midway between neighbours
    e = Engine(precision="fp16", max_batch=B, max_det=300, num_classes=91, det_input=S)
    try:
        e.load_detector(p, b)
        s = np.sort(e.detect_raw(imgs)[:, 4:].max(axis=1).astype(np.float64).ravel())[::-1]
    finally:
        e.close()
    k = PER_IMAGE * B
    mid = 0.5 * (np.log(s[k - 1] / (1 - s[k - 1])) + np.log(s[k] / (1 - s[k])))
    ncnn_export.shift_cls_bias(p, b, float(np.log(CONF / (1 - CONF)) - mid), nc=nc)
    # max_det: at conf 0.001 more boxes survive the NMS than the default 300 (the anchors of either shape are fewer than MAX_DET)
    eng = Engine(precision="fp16", max_batch=B, max_det=MAX_DET, num_classes=91, det_input=S, max_rois=256)
    try:
        eng.load_detector(p, b)
        eng.load_classifier(random_shufflenet_state(91, seed=3))
        out0 = eng.detect_raw(imgs)
        out0.setflags(write=False)
        yield eng, imgs, out0
    finally:
        eng.close()


def test_calibrated_most_tiles_leave(setup):
    eng, imgs, out0 = setup
    passing = (out0[:, 4:].max(axis=1) > CONF).sum(axis=1)
    print(f"anchors above conf per image: {passing.tolist()} of {out0.shape[2]}")
    assert 0 < passing.sum() <= 2 * PER_IMAGE * len(imgs)
    kept = _check_detect(eng, imgs, out0, CONF, "calibrated")
    assert max(kept) >= 1, "no image has a kept box: the test would be vacuous"


def test_every_tile_leaves_then_calibrated(setup):
    eng, imgs, out0 = setup
    assert (out0[:, 4:] <= 0.999).all()
    _, counts = eng.detect(list(imgs), 0.999, IOU)
    assert (counts == 0).all(), counts
    kept = _check_detect(eng, imgs, out0, CONF, "0.25 after 0.999")   # no state survives; the vote word is per workgroup
    assert max(kept) >= 1


def test_no_tile_leaves(setup):
    eng, imgs, out0 = setup
    assert (out0[:, 4:].max(axis=1) > 0.001).any(axis=1).all()
    _check_detect(eng, imgs, out0, 0.001, "conf 0.001")


def test_device_path_eager_and_graph_replay(setup):
    from litepi._ffi import DET_DTYPE
    from litepi.distributed import alloc_result_buffers
    eng, imgs, out0 = setup
    B, S = imgs.shape[0], imgs.shape[1]
    dev = torch.device("cuda", 0)
    dimg = torch.from_numpy(imgs).to(dev)
    res = alloc_result_buffers(B, MAX_DET, dev)
    want = [len(eb) for eb, _, _ in _reference(out0, S, CONF)]
    runs = []
    for _ in range(3):   # first sight of the input pointer (eager), capture, replay
        eng.run_batch_device(dimg.data_ptr(), B, S, S, CONF, IOU, 0, res.dets.data_ptr(), res.counts.data_ptr())
        eng.synchronize()
        torch.cuda.synchronize()
        counts = res.counts.cpu().numpy().copy()
        recs = res.dets.cpu().numpy().reshape(B, -1).view(DET_DTYPE).reshape(B, -1).copy()
        assert counts[B:2 * B].tolist() == want, f"boxes after NMS: {counts[B:2 * B].tolist()} vs {want}"
        runs.append((counts, [recs[i, :counts[i]].tobytes() for i in range(B)]))
    assert sum(want) >= 1
    for k in (1, 2):
        assert np.array_equal(runs[0][0], runs[k][0]) and runs[0][1] == runs[k][1], f"call {k} differs from the first"


# What a fresh process does for test_workgroups_leave_on_every_v1_shape: the kernel shape switches are read per load, but
# LITEPI_HEAD_STAMPS once per process, so each switch runs in a process of its own.  LITEPI_HEAD_STAMPS makes every head launch append a record
# [magic, grid, H, N][grid][16] whose stamp 14 is 1 for a workgroup that left at the vote.
_STAMP_SCRIPT = r"""
import json, os, sys
import numpy as np
from litepi import Engine, ncnn_export
from oracle import postprocess_ref as P
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
out0 = e.detect_raw(imgs)

def levels():
    raw = np.fromfile(stamps, dtype=np.uint64)
    open(stamps, "wb").close()
    out, off = [], 0
    while off < len(raw):
        assert raw[off] == 0x48454144
        grid, H = int(raw[off + 1]), int(raw[off + 2])
        st = raw[off + 4: off + 4 + grid * 16].reshape(grid, 16)
        out.append({"H": H, "grid": grid, "left": int((st[:, 14] == 1).sum())})
        off += 4 + grid * 16
    return out

raw_levels = levels()[-3:]
res = {"raw": raw_levels, "runs": {}}
for conf in (0.25, 0.999, 0.001):
    dets, counts = e.detect(list(imgs), conf, 0.45)
    same = True
    for i in range(B):
        eb, es, ec = P.postprocess(out0[i], (S, S), 1.0, (0.0, 0.0), conf, 0.45)
        same = same and counts[i] == len(eb) and all(
            float(dets[i, j]["det_conf"]) == float(es[j]) and
            tuple(int(dets[i, j][f]) for f in ("x1", "y1", "x2", "y2")) == tuple(int(v) for v in eb[j].astype(int)) for j in range(len(eb)))
    res["runs"][str(conf)] = {"levels": levels(), "same": bool(same), "kept": int(counts.sum())}
n = [(S // 8) ** 2, (S // 16) ** 2, (S // 32) ** 2]
edges = np.cumsum([0] + n)
res["passing"] = [int((out0[:, 4, edges[l]:edges[l + 1]] > 0.25).sum()) for l in range(3)]
e.close()
print("RESULT " + json.dumps(res))
"""


@pytest.mark.parametrize("switch", ["", "LITEPI_HEAD_A32", "LITEPI_HEAD_2WG", "LITEPI_HEAD_1WG"], ids=lambda s: s or "default")
def test_workgroups_leave_on_every_v1_shape(tmp_path, switch):
    """The early exit really happens, and on every v1 shape ``HeadLayer::launch`` can reach: the default ones and those behind
    the A/B switches (round 3's stage A, the two-workgroup shapes -- whose P3 LDS is exactly its 80 KiB limit --, the
    one-workgroup shapes).  With stamps on, a calibrated detect must show workgroups that left AND workgroups that stayed (never
    more stayers on a level than it has anchors above conf), conf 0.999 only leavers, the parity hook none; and the records
    must still equal the postprocess of the same handle's out0."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("LITEPI_HEAD_")}
    env.update(LITEPI_HEAD_STAMPS=str(tmp_path / "stamps.bin"), LITEPI_NO_GRAPH="1",
               PYTHONPATH=os.pathsep.join([os.path.join(root, "yolo-litepi_amd"), root, env.get("PYTHONPATH", "")]))
    if switch:
        env[switch] = "1"
    r = subprocess.run([sys.executable, "-c", _STAMP_SCRIPT, str(tmp_path)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(switch or "default", res)
    assert [lv["H"] for lv in res["raw"]] == [40, 20, 10] and all(lv["left"] == 0 for lv in res["raw"]), "the parity hook must never leave"
    cal, none, every = (res["runs"][c] for c in ("0.25", "0.999", "0.001"))
    assert cal["same"] and none["same"] and every["same"]
    assert cal["kept"] >= 1 and none["kept"] == 0
    for lv, passing in zip(cal["levels"], res["passing"]):
        stayed = lv["grid"] - lv["left"]
        assert (stayed >= 1) == (passing >= 1) and stayed <= passing, (lv, passing)
    assert sum(lv["left"] for lv in cal["levels"]) >= 1 and sum(res["passing"]) >= 1
    assert all(lv["left"] == lv["grid"] for lv in none["levels"]), none
    assert sum(lv["grid"] - lv["left"] for lv in every["levels"]) > sum(lv["grid"] - lv["left"] for lv in cal["levels"])
