"""GPU tests of crop quality (include/litepi.h, lp_quality), everything through the C-ABI: the measure kernel alone
against the NumPy restatement of the rule (tests/quality_ref.py) bit for bit, the argument and state errors, the inventory
under the sharpness rank against InventorySharpRef (with and without an evidence store), and the records every pipeline
family leaves.  No tolerance anywhere: every reduction is over integers."""
import ctypes as C

import numpy as np
import pytest
import torch

import quality_ref as Q
import tracking_ref as R

pytestmark = pytest.mark.gpu

MB, MD = 4, 10   # B * max_det = 40 records


def named_crops(S, R_):
    """R_ crops of size S: the random, extreme and sign crops of the CPU test first, further noise behind them"""
    base = list(Q.shared_crops(S).values())
    return np.stack([base[r] if r < len(base) else Q.noise_crop(S, 10 + r) for r in range(R_)]) if R_ else np.zeros((0, S, S, 3), np.uint8)


# ---------------------------------------------------------------------------- 1. the measure kernel alone
# 8, 36, 64, 224: one strip with units that straddle rows (36), two strips (224).  188 and 372: two and five strips with
# S % 8 == 4, where a strip's lower halo row ends in the middle of a 16-pixel unit
@pytest.mark.parametrize("S", (8, 36, 64, 188, 224, 372))
def test_measure_kernel_equals_the_rule(S):
    from litepi import Engine
    eng = Engine(precision="fp16", max_batch=MB, max_det=MD, num_classes=4, cls_input=S)
    try:
        eng.quality_enable(True)
        dev = eng.quality_buffer()
        assert dev != 0 and dev % 16 == 0
        assert Q.is_empty(eng.quality_read(MB)).all(), "the buffer is cleared to the empty record at allocation"
        rng = np.random.default_rng(S)
        every = np.arange(MB * MD)
        sent_crops = np.stack([Q.noise_crop(S, 100 + r % 3) for r in every])
        for R_, B in ((0, 1), (0, MB), (1, 1), (1, MB), (3, 2), (3, MB), (MD, 1), (40, MB)):
            eng.test_set_rois(sent_crops, every // MD, every % MD)   # the sentinel: every record of all frames measured
            sentinel = eng.test_quality(MB)
            assert not Q.is_empty(sentinel).any()
            crops = named_crops(S, R_)
            where = rng.permutation(B * MD)[:R_]   # a random injective map ROI -> (frame, slot), in no order
            img, slot = where // MD, where % MD
            eng.test_set_rois(crops, img, slot)
            got = eng.test_quality(B)
            want = Q.records_for(crops, img, slot, B, MD)
            assert got.shape == (B, MD) and got.tobytes() == want.tobytes(), (S, R_, B, got[got != want], want[got != want])
            assert Q.is_empty(got).sum() == B * MD - R_
            both = eng.quality_read(MB)
            assert both[:B].tobytes() == want.tobytes() and both[B:].tobytes() == sentinel[B:].tobytes(), \
                f"S {S} R {R_} B {B}: the records of frames >= B must be left alone"
        # B = 2 on a list that also names frames 2 and 3: those ROIs are skipped, their records keep the bytes of the call before
        eng.test_set_rois(sent_crops, every // MD, every % MD)
        sentinel = eng.test_quality(MB)
        crops = named_crops(S, 12)
        where = rng.permutation(MB * MD)[:12]
        img, slot = where // MD, where % MD
        assert (img >= 2).any() and (img < 2).any()
        eng.test_set_rois(crops, img, slot)
        got = eng.test_quality(2)
        assert got.tobytes() == Q.records_for(crops, img, slot, 2, MD).tobytes()
        assert eng.quality_read(MB)[2:].tobytes() == sentinel[2:].tobytes()
        assert eng.quality_buffer() == dev
    finally:
        eng.close()


# ---------------------------------------------------------------------------- 2. errors
def test_errors_leave_the_handle_usable():
    from litepi import Engine, _ffi
    S = 8
    eng = Engine(precision="fp16", max_batch=MB, max_det=MD, num_classes=4, cls_input=S)
    odd = Engine(precision="fp16", max_batch=1, max_det=MD, num_classes=4, cls_input=30)
    lib, h = eng.lib, eng._h
    ip, vp = C.POINTER(C.c_int), C.c_void_p
    try:
        rec = np.zeros((MB, MD), dtype=_ffi.QUALITY_DTYPE)
        assert lib.lp_quality_enable(odd._h, 1) == _ffi.LP_ERR_STATE and b"multiple of 4" in lib.lp_last_error()
        assert lib.lp_quality_enable(odd._h, 0) == 0   # nothing to change
        for on in (-1, 2):
            assert lib.lp_quality_enable(h, on) == _ffi.LP_ERR_ARG
        p = vp()
        assert lib.lp_quality_buffer(h, C.byref(p)) == _ffi.LP_ERR_STATE
        assert lib.lp_quality_read(h, rec.ctypes.data, 1) == _ffi.LP_ERR_STATE
        assert lib.lp_test_quality(h, 1, rec.ctypes.data) == _ffi.LP_ERR_STATE
        assert lib.lp_inventory_set_rank(h, _ffi.LP_RANK_SHARPNESS) == _ffi.LP_ERR_STATE   # no tracker, no inventory
        eng.tracker_create(max_tracks=4)
        assert lib.lp_inventory_set_rank(h, _ffi.LP_RANK_CONFIG) == _ffi.LP_ERR_STATE      # no inventory
        eng.inventory_create()
        assert lib.lp_inventory_set_rank(h, _ffi.LP_RANK_SHARPNESS) == _ffi.LP_ERR_STATE   # quality off
        assert lib.lp_inventory_set_rank(h, _ffi.LP_RANK_CONFIG) == 0
        eng.quality_enable(True)
        addr = eng.quality_buffer()
        # the valid call that must give the same records after every refusal
        crops = named_crops(S, 3)
        img, slot = np.array([1, 0, 1], np.int32), np.array([4, 2, 0], np.int32)
        eng.test_set_rois(crops, img, slot)
        want = Q.records_for(crops, img, slot, 2, MD)

        def still_works():
            assert eng.test_quality(2).tobytes() == want.tobytes() and eng.quality_read(2).tobytes() == want.tobytes()
        still_works()
        for B in (0, MB + 1, -1):
            assert lib.lp_quality_read(h, rec.ctypes.data, B) == _ffi.LP_ERR_ARG
            assert lib.lp_test_quality(h, B, rec.ctypes.data) == _ffi.LP_ERR_ARG
            still_works()
        assert lib.lp_quality_read(h, None, 1) == _ffi.LP_ERR_ARG and lib.lp_test_quality(h, 1, None) == _ffi.LP_ERR_ARG
        still_works()
        for on in (-1, 2):
            assert lib.lp_quality_enable(h, on) == _ffi.LP_ERR_ARG
        still_works()
        for rank in (2, -1):
            assert lib.lp_inventory_set_rank(h, rank) == _ffi.LP_ERR_ARG
        with pytest.raises(ValueError):
            eng.inventory_set_rank("biggest")
        still_works()
        dets, tracks = np.zeros((2, MD), dtype=_ffi.DET_DTYPE), np.zeros((2, MD), dtype=_ffi.TRACK_DTYPE)
        counts = np.zeros(2, np.int32)

        def inv_host(crops_flag):
            return lib.lp_inventory(h, dets.ctypes.data, counts.ctypes.data_as(ip), tracks.ctypes.data, 2, None, crops_flag)
        d = torch.zeros(2 * MD * 32, dtype=torch.uint8, device="cuda")
        c = torch.zeros(2, dtype=torch.int32, device="cuda")
        t = torch.zeros(2 * MD * 32, dtype=torch.uint8, device="cuda")

        def inv_dev(crops_flag):
            return lib.lp_inventory_device(h, vp(d.data_ptr()), vp(c.data_ptr()), vp(t.data_ptr()), 2, None, crops_flag)
        assert inv_host(0) == 0 and inv_dev(0) == 0   # LP_RANK_CONFIG: crops = 0 is fine
        eng.inventory_set_rank("sharpness")
        assert inv_host(0) == _ffi.LP_ERR_ARG and b"crops = 0" in lib.lp_last_error()
        assert inv_dev(0) == _ffi.LP_ERR_ARG
        still_works()
        assert inv_host(1) == 0 and inv_dev(1) == 0
        assert lib.lp_quality_enable(h, 0) == _ffi.LP_ERR_STATE and b"sharpness" in lib.lp_last_error()
        assert lib.lp_quality_enable(h, 1) == 0   # no change
        eng.synchronize()
        assert eng.quality_read(2).tobytes() == want.tobytes(), "a refused call must not touch the records"
        still_works()
        eng.inventory_set_rank("config")
        assert inv_host(0) == 0
        eng.quality_enable(False)
        assert lib.lp_quality_buffer(h, C.byref(p)) == _ffi.LP_ERR_STATE
        eng.quality_enable(True)
        assert eng.quality_buffer() == addr, "the buffer's address is stable until lp_destroy"
        assert eng.test_quality(2).tobytes() == want.tobytes()
        assert len(eng.inventory_drain()[0]) == 0
    finally:
        eng.close()
        odd.close()


# ---------------------------------------------------------------------------- 3. the inventory under the sharpness rank
INV_S, INV_MD, INV_FRAMES, INV_HW = 64, 8, 6, 160


def inventory_case():
    """Four hand-made tracks of six frames on one stream, record i of every frame = track i + 1 in slot i, every box growing
    from frame to frame (by area the last frame is the best).  The crops, by frame:
      track 1  blurred sign, sign, sign + noise, sign + more noise (sharpness rising), then twice the doubly blurred sign
      track 2  sign, blurred sign, then no crop at all: a sighting without a crop never replaces the best
      track 3  no crop, sign, then blurred signs: the unmeasured first sighting is replaced by the first measured one
      track 4  the same sign in every frame: a tie keeps the earlier sighting"""
    sign = Q.sign_crop(INV_S)
    b1 = Q.box_blur(sign)
    b2 = Q.box_blur(b1)
    rng = np.random.default_rng(5)

    def noisy(amp):
        return np.clip(sign.astype(np.int64) + rng.integers(-amp, amp + 1, sign.shape), 0, 255).astype(np.uint8)
    per_track = [[b1, sign, noisy(6), noisy(20), b2, b2], [sign, b1, None, None, None, None], [None, sign, b1, b1, b2, b2], [sign] * 6]
    rising = [float(Q.measure(c)["sharpness"]) for c in per_track[0]]
    assert rising[0] < rising[1] < rising[2] < rising[3] and rising[4] == rising[5] < rising[0], rising   # of the reference, not the device
    dets, tracks = np.zeros((INV_FRAMES, INV_MD), dtype=R.DET_DTYPE), np.zeros((INV_FRAMES, INV_MD), dtype=R.TRACK_DTYPE)
    crops = {}
    for f in range(INV_FRAMES):
        for k in range(4):
            dets[f, k] = (20.0 + 35 * k - f, 40.0 - f, 36.0 + 35 * k + f, 60.0 + f, 0.9 - 0.01 * f, k, 5 + k, 0.8)
            tr = tracks[f, k]
            tr["track_id"], tr["slot"], tr["hits"], tr["voted_class"], tr["voted_conf"], tr["vote_weight"] = k + 1, k, f + 1, 5 + k, 0.8, f + 1
            if per_track[k][f] is not None:
                crops[(f, k)] = per_track[k][f]
    counts = np.full(INV_FRAMES, 4, np.int32)
    keys = list(crops)
    order = np.random.default_rng(9).permutation(len(keys))   # the ROI list in no order
    img, slot = np.array([keys[o][0] for o in order], np.int32), np.array([keys[o][1] for o in order], np.int32)
    roi_crops = np.stack([crops[keys[o]] for o in order])
    frames = np.random.default_rng(11).integers(0, 256, (INV_FRAMES, INV_HW, INV_HW, 3), dtype=np.uint8)
    return dict(dets=dets, tracks=tracks, counts=counts, crops=crops, img=img, slot=slot, roi_crops=roi_crops, frames=frames, per_track=per_track)


@pytest.fixture(scope="module")
def inv_engine():
    from litepi import Engine
    eng = Engine(precision="fp16", max_batch=8, max_det=INV_MD, num_classes=16, cls_input=INV_S)
    eng.quality_enable(True)
    yield eng
    eng.close()


@pytest.mark.parametrize("evidence", (False, True), ids=("plain", "evidence"))
@pytest.mark.parametrize("rank", ("sharpness", "config"))
def test_inventory_under_the_rank_equals_the_reference(inv_engine, rank, evidence):
    from litepi import _ffi, backend
    eng, cs = inv_engine, inventory_case()
    tcfg = dict(max_tracks=8, max_age=2, min_hits=2)
    eng.tracker_create(**tcfg)
    eng.inventory_create()
    if evidence:
        eng.evidence_create(size=32, scale=2.0)
        eng.test_set_frames(cs["frames"])
    eng.inventory_set_rank(rank)
    eng.test_set_rois(cs["roi_crops"], cs["img"], cs["slot"])
    quality = eng.test_quality(INV_FRAMES)
    want_q = Q.records_for(cs["roi_crops"], cs["img"], cs["slot"], INV_FRAMES, INV_MD)
    assert quality.tobytes() == want_q.tobytes()
    eng.inventory(cs["dets"], cs["counts"], cs["tracks"], crops=True)
    eng.inventory_flush(-1)
    if evidence:
        signs, crops, pics, wins, dropped = eng.inventory_drain_evidence()
    else:
        signs, crops, dropped = eng.inventory_drain()
    ref = Q.InventorySharpRef(max_det=INV_MD, track_cfg=tcfg, crop_size=INV_S)
    ref.feed(cs["dets"], cs["tracks"], cs["counts"], crops=cs["crops"], quality=want_q if rank == "sharpness" else None)
    ref.flush()
    want, want_crops, _ = ref.drain()
    assert dropped == 0 and len(signs) == len(want) == 4
    plain = signs.copy()
    plain["flags"] &= ~_ffi.LP_SIGN_HAS_EVIDENCE
    assert plain.tobytes() == want.tobytes(), (rank, plain, want)
    assert crops.tobytes() == want_crops.tobytes()
    if rank == "sharpness":
        assert signs["best_frame"].tolist() == [3, 0, 1, 0]
        for k, f in enumerate(signs["best_frame"]):
            crop = cs["per_track"][k][f]
            assert signs["best_quality"][k].tobytes() == Q.measure(crop)["sharpness"].tobytes() and crops[k].tobytes() == crop.tobytes()
            assert signs["flags"][k] & _ffi.LP_SIGN_HAS_CROP
    else:
        assert signs["best_frame"].tolist() == [5, 5, 5, 5]
        assert [bool(fl & _ffi.LP_SIGN_HAS_CROP) for fl in signs["flags"]] == [True, False, True, True]
    if evidence:   # the window logged with the sign is that of the same sighting
        for k, f in enumerate(signs["best_frame"]):
            d = cs["dets"][f, k]
            win, has = backend.evidence_window(eng.ev_cfg, INV_HW, INV_HW, (d["x1"], d["y1"], d["x2"], d["y2"]))
            assert has and bool(signs["flags"][k] & _ffi.LP_SIGN_HAS_EVIDENCE) and tuple(int(v) for v in wins[k]) == win, (rank, k, f)
        assert len({tuple(w) for w in wins.tolist()}) == 4 and pics.any()


# ---------------------------------------------------------------------------- 4. the rank does not outlive its inventory
def test_inventory_create_restores_the_config_rank(inv_engine):
    from litepi import _ffi
    eng, cs = inv_engine, inventory_case()
    eng.tracker_create(max_tracks=8, max_age=2, min_hits=2)
    eng.inventory_create()
    eng.inventory_set_rank("sharpness")
    assert eng.lib.lp_quality_enable(eng._h, 0) == _ffi.LP_ERR_STATE
    eng.inventory_create()   # again: LP_RANK_CONFIG
    eng.test_set_rois(cs["roi_crops"], cs["img"], cs["slot"])
    eng.test_quality(INV_FRAMES)
    eng.inventory(cs["dets"], cs["counts"], cs["tracks"], crops=False)   # refused under the sharpness rank
    eng.inventory(cs["dets"], cs["counts"], cs["tracks"], crops=True)
    assert eng.inventory_open(0)["best_frame"].tolist() == [5, 5, 5, 5]   # by area: the second call's boxes repeat the first's, and a tie keeps the earlier sighting
    eng.quality_enable(False)   # refused while ranked
    eng.quality_enable(True)


# ---------------------------------------------------------------------------- 5. through the pipeline
CONF, IOU, MIN_AREA = 0.25, 0.45, 50
N_CALLS, N_FRAMES, NC_PIPE, TOPK = 6, 2, 91, 5


def moving_patch(base, rng, step=4):
    """N_CALLS versions of the frames `base` with a pasted patch that moves `step` pixels to the right per call"""
    patch = rng.integers(0, 256, (96, 96, 3), dtype=np.uint8)
    out = []
    for k in range(N_CALLS):
        f = base.copy()
        f[:, 200:296, 160 + step * k:256 + step * k] = patch
        out.append(f)
    return out


@pytest.fixture(scope="module")
def clip():
    rng = np.random.default_rng(77)
    return moving_patch(rng.integers(0, 256, (N_FRAMES, 640, 640, 3), dtype=np.uint8), rng)


@pytest.fixture(scope="module")
def models(tmp_path_factory, clip):
    """a seeded v1 detector whose class bias is shifted so that on the first and the last call's frames at least three anchors
    pass conf 0.25 with a margin of 0.1 in the logit, measured with the device's own scores (as tests/test_gpu_topk.py), and a
    seeded classifier"""
    from litepi import Engine, ncnn_export
    from litepi.backend import random_shufflenet_state
    d = tmp_path_factory.mktemp("quality_models")
    sd = random_shufflenet_state(NC_PIPE, seed=3)
    cls_file = str(d / "cls.pth")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, cls_file)
    every = [f for k in (0, N_CALLS - 1) for f in clip[k]]
    p, b = str(d / "v1.param"), str(d / "v1.bin")
    ncnn_export.export_detector(p, b, "v1", seed=4321, cls_bias=0.0)
    e = Engine(precision="fp16", max_batch=len(every), max_det=300, num_classes=NC_PIPE)
    try:
        e.load_detector(p, b)
        lb = np.stack([e.test_letterbox(f)[0] for f in every])
        s = np.sort(e.detect_raw(lb)[:, 4:].max(axis=1).astype(np.float64), axis=1)[:, ::-1]
    finally:
        e.close()
    third = s[:, 2].min()
    ncnn_export.shift_cls_bias(p, b, float(np.log(0.25 / 0.75) - (np.log(third / (1 - third)) - 0.1)))
    return {"cls": sd, "cls_file": cls_file, "v1": (p, b)}


def _engine(models, prec="fp16", max_batch=4, max_rois=0):
    from litepi import Engine
    e = Engine(precision=prec, max_batch=max_batch, max_det=300, num_classes=NC_PIPE, max_rois=max_rois)
    e.load_detector(*models["v1"])
    e.load_classifier(models["cls"])
    return e


def check_records(dets, counts, quality, rois, tag):
    """(b): every record the ROI list names equals quality_measure of its crop; every other record of the frames is empty.
    Returns the number of measured records."""
    from litepi import backend
    crops, img, slot = rois
    named = {(int(b), int(i)): r for r, (b, i) in enumerate(zip(img, slot))}
    for b in range(len(counts)):
        for i in range(dets.shape[1]):
            q = quality[b, i]
            if (b, i) in named:
                assert i < counts[b] and dets[b, i]["cls_class"] >= 0, f"{tag}: the ROI list names record ({b}, {i}), which is not classified"
                want = backend.quality_measure(crops[named[(b, i)]])
                assert q.tobytes() == want.tobytes() == Q.measure(crops[named[(b, i)]]).tobytes(), f"{tag}: record ({b}, {i}): {q} != {want}"
            else:
                assert not (i < counts[b] and dets[b, i]["cls_class"] >= 0), f"{tag}: classified record ({b}, {i}) has no ROI"
                assert Q.is_empty(q[None])[0], f"{tag}: record ({b}, {i}) must be empty"
    return len(named)


@pytest.fixture(scope="module")
def piped(models, clip):
    """one fp16 handle (max_batch 4, 2 frames): the device step with quality off, on and off again, then with top-k on as well --
    records, launch lists, graph counters -- and what the other checks need of the `on` state"""
    from litepi._ffi import DET_DTYPE
    dev = torch.device("cuda", 0)
    eng = _engine(models)
    B = N_FRAMES
    x = torch.from_numpy(clip[0]).to(dev)
    d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device=dev)
    c = torch.zeros(3 * B, dtype=torch.int32, device=dev)
    out = {"eng": eng, "x": x, "states": []}

    def step():
        eng.run_batch_device(x.data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())

    def fetch():
        eng.synchronize()
        return d.cpu().numpy().copy(), c.cpu().numpy().copy()
    try:
        for on, k in ((False, 0), (True, 0), (False, 0), (True, TOPK)):
            eng.quality_enable(on)
            eng.topk_enable(k)
            before = eng.graph_stats()
            for _ in range(3):   # eager, capture, replay
                step()
            eng.synchronize()
            st = {"on": on, "k": k, "bytes": tuple(a.tobytes() for a in fetch()), "first3": (before, eng.graph_stats())}
            if on:
                before = eng.graph_stats()
                for _ in range(10):
                    step()
                eng.synchronize()
                st["stats"] = (before, eng.graph_stats())
                st["bytes10"] = tuple(a.tobytes() for a in fetch())
                st["quality"] = eng.quality_read(B)
                st["rois"] = eng.debug_rois()
                st["overflow"] = eng.roi_overflow()
            eng.profile_next(True)
            step()
            eng.synchronize()
            st["launches"] = [(r["name"], r["layer"]) for r in eng.profile_read()]
            st["bytes_profiled"] = tuple(a.tobytes() for a in fetch())
            if on:
                st["quality_profiled"] = eng.quality_read(B)
            out["states"].append(st)
        dn, cn = fetch()
        out["dets"], out["counts"] = dn.view(DET_DTYPE).reshape(B, 300), cn[:B]
        eng.topk_enable(0)
        yield out
    finally:
        eng.close()


def test_records_are_the_same_off_on_and_off_again(piped):   # (a)
    off, on, off2, both = piped["states"]
    assert off["bytes"] == on["bytes"] == off2["bytes"] == both["bytes"], "lp_det records or counts differ with quality on"
    assert on["bytes10"] == on["bytes"] and on["bytes_profiled"] == on["bytes"] and off["bytes_profiled"] == off["bytes"]
    assert piped["counts"].min() >= 1


def test_quality_records_of_the_device_step(piped):   # (b)
    on, both = piped["states"][1], piped["states"][3]
    n = check_records(piped["dets"], piped["counts"], on["quality"], on["rois"], "device")
    assert n == piped["counts"].sum() >= 2 and on["overflow"] == (n, n)
    assert on["quality_profiled"].tobytes() == on["quality"].tobytes(), "the eager profiled step leaves other records than the replayed one"
    assert both["quality"].tobytes() == on["quality"].tobytes(), "top-k on changes the quality records"
    valid = on["quality"][on["quality"]["flags"] == Q.VALID]
    assert len(valid) == n and (valid["sharpness"] > 0).all() and (valid["luma_mean"] > 0).all()


def test_unclassified_kept_records_are_empty(piped, models):   # (b), a user-set max_rois
    from litepi._ffi import DET_DTYPE
    B = N_FRAMES
    eng = _engine(models, max_rois=1)
    try:
        eng.quality_enable(True)
        d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
        c = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        eng.run_batch_device(piped["x"].data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
        classified, kept = eng.roi_overflow()
        assert classified == 1 and kept >= 2
        dets, counts = d.cpu().numpy().view(DET_DTYPE).reshape(B, 300), c.cpu().numpy()[:B]
        quality = eng.quality_read(B)
        assert check_records(dets, counts, quality, eng.debug_rois(), "max_rois = 1") == 1
        assert Q.is_empty(quality).sum() == B * 300 - 1
    finally:
        eng.close()


def test_no_classifier_leaves_every_record_empty(piped, models):
    from litepi import Engine
    B = N_FRAMES
    eng = Engine(precision="fp16", max_batch=4, max_det=300, num_classes=NC_PIPE)
    try:
        eng.load_detector(*models["v1"])
        eng.quality_enable(True)
        d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
        c = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
        for _ in range(3):
            eng.run_batch_device(piped["x"].data_ptr(), B, 640, 640, CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
        quality = eng.quality_read(B)   # synchronises the engine's stream
        assert c.cpu().numpy()[:B].min() >= 1 and Q.is_empty(quality).all()
    finally:
        eng.close()


def test_views_and_host_calls_index_records_by_frame(piped, clip):   # (c)
    from litepi._ffi import DET_DTYPE
    eng, B = piped["eng"], N_FRAMES
    d = torch.zeros(B * 300 * 32, dtype=torch.uint8, device="cuda")
    c = torch.zeros(3 * B, dtype=torch.int32, device="cuda")
    eng.run_views_device(piped["x"].data_ptr(), B, 640, 640, ["full", (128, 128, 384, 384)], CONF, IOU, MIN_AREA, d.data_ptr(), c.data_ptr())
    quality = eng.quality_read(B)
    dets, counts = d.cpu().numpy().view(DET_DTYPE).reshape(B, 300), c.cpu().numpy()[:B]
    assert check_records(dets, counts, quality, eng.debug_rois(), "views") >= 2 and counts.min() >= 1
    hd, hc, _, timing = eng.run_batch(list(clip[0]), CONF, IOU, MIN_AREA)
    quality = eng.quality_read(B)
    assert check_records(hd[:B], hc[:B], quality, eng.debug_rois(), "host") == piped["counts"].sum()
    assert quality.tobytes() == piped["states"][1]["quality"].tobytes(), "the host call leaves other records than the device call"
    assert timing.t_classification > 0


def test_repeated_steps_are_replays_and_toggling_recaptures(piped):   # (d)
    for st in piped["states"]:
        before, after = st["first3"]   # every toggle: eager, capture, replay of a new step
        assert (after["eager"] - before["eager"], after["captures"] - before["captures"], after["replays"] - before["replays"]) == (1, 1, 1), st["on"]
    for st in (piped["states"][1], piped["states"][3]):
        before, after = st["stats"]
        assert after["replays"] - before["replays"] == 10 and after["eager"] == before["eager"] and after["captures"] == before["captures"]


def test_launch_lists(piped):   # (e)
    off, on, off2, both = (s["launches"] for s in piped["states"])
    assert off == off2 and len(off) > 10, "a handle switched on and off again must run the launches it ran before"
    assert not any("quality" in name or layer == "quality" for name, layer in off)
    assert [x for x in on if x[1] != "quality"] == off, "quality on must add launches only"
    assert [x for x in on if x[1] == "quality"] == [("quality_clear", "quality"), ("quality_measure", "quality")]
    assert on[-2:] == [("quality_clear", "quality"), ("quality_measure", "quality")]
    assert [x for x in both if x[1] == "quality"] == [("quality_clear", "quality"), ("quality_measure", "quality")]
    assert {n for n, layer in both if layer == "topk"} == {"topk_clear", "topk_select"}
    assert [x for x in both if x[1] not in ("quality", "topk")] == off


def test_pipeline_result_dicts(models, clip):   # (f)
    from litepi import HybridPipeline
    from litepi.backend import QUALITY_RESULT_KEYS
    kw = dict(num_classes=NC_PIPE, precision="fp16", max_batch=4)
    keys = {}
    for quality in (False, True):
        pipe = HybridPipeline(*models["v1"], models["cls_file"], "shufflenetv2", quality=quality, **kw)
        try:
            outs = pipe.run_batch(list(clip[0]), CONF, IOU, MIN_AREA)
            keys[quality] = {frozenset(r) for res, _ in outs for r in res}
            assert sum(len(res) for res, _ in outs) >= 2
            if quality:
                rec = pipe.engine.quality_read(N_FRAMES)
                for b, (res, _) in enumerate(outs):
                    for i, r in enumerate(res):
                        q = rec[b, i]
                        assert q["flags"] == Q.VALID and all(isinstance(r[k], float) for k in QUALITY_RESULT_KEYS)
                        assert [r[k] for k in QUALITY_RESULT_KEYS] == [float(q[k]) for k in QUALITY_RESULT_KEYS], (b, i)
        finally:
            pipe.close()
    assert len(keys[False]) == len(keys[True]) == 1
    (without,), (with_,) = keys[False], keys[True]
    assert with_ - without == set(QUALITY_RESULT_KEYS) and without - with_ == set() and not without & set(QUALITY_RESULT_KEYS)


def test_pipeline_inventory_ranks_by_sharpness(models, clip):
    from litepi import HybridPipeline
    tcfg = dict(n_streams=N_FRAMES, max_tracks=64, max_age=0, min_hits=1, iou_match=0.5)
    pipe = HybridPipeline(*models["v1"], models["cls_file"], "shufflenetv2", num_classes=NC_PIPE, precision="fp16", max_batch=4,
                          track=True, track_config=tcfg, inventory=dict(best="sharpness"))
    try:
        assert pipe.quality and pipe.engine.inv_cfg.best == 0
        seen = {}
        for frames in clip[:3]:
            outs = pipe.run_batch(list(frames), CONF, IOU, MIN_AREA, stream_ids=np.arange(N_FRAMES, dtype=np.int32))
            for b, (res, _) in enumerate(outs):
                for r in res:
                    assert r["sharpness"] is not None
                    seen.setdefault((b, r["track_id"]), []).append(np.float32(r["sharpness"]))
        signs = pipe.drain_signs(flush=True)
        assert len(signs) >= 2
        assert pipe.engine.lib.lp_quality_enable(pipe.engine._h, 0) != 0, "quality cannot be switched off while the inventory ranks by sharpness"
        for s in signs:   # the first of the sharpest sightings, and its crop's measure is that sharpness
            sh = seen[(s["stream"], s["track_id"])]
            assert s["best_frame"] - s["first_frame"] == int(np.argmax(sh)), (s["track_id"], sh)
            assert Q.measure(s["crop"])["sharpness"] == max(sh)
    finally:
        pipe.close()
