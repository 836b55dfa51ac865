"""NumPy float32 restatement of the tracking rule of include/litepi.h (lp_track_config) and the scene generators of the
tracking tests.  Nothing in the reference tracks, so this file is what pins liblitepi_hip's tracker: every fp32 operation is
written out on its own, in the header's order, so the device result must be bit-equal.

    ref = TrackerRef(max_det=16, num_classes=58, max_tracks=8)
    tracks = ref.track(dets, counts)            # dets [B, max_det] lp_det records, counts [B] -> [B, max_det] lp_track records
    snap = ref.snapshot(0)                      # {"tracks": ..., "acc": ..., "next_id": ..., "overflow": ...}
"""
from __future__ import annotations

import numpy as np

DET_DTYPE = [("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("det_conf", "<f4"), ("det_class", "<i4"),
             ("cls_class", "<i4"), ("cls_conf", "<f4")]
TRACK_DTYPE = [("track_id", "<i4"), ("slot", "<i4"), ("hits", "<i4"), ("age", "<i4"), ("voted_class", "<i4"), ("voted_conf", "<f4"),
               ("vote_weight", "<f4"), ("flags", "<i4")]
TRACK_STATE_DTYPE = [("slot", "<i4"), ("track_id", "<i4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("vx1", "<f4"),
                     ("vy1", "<f4"), ("vx2", "<f4"), ("vy2", "<f4"), ("hits", "<i4"), ("missed", "<i4"), ("age", "<i4"),
                     ("det_class", "<i4"), ("wsum", "<f4"), ("has_vote", "<i4")]
CONFIRMED, BORN = 1, 2
F = np.float32
EPS = F(1e-6)

DEFAULTS = dict(n_streams=1, max_tracks=64, iou_match=0.3, max_age=5, min_hits=3, new_conf=0.0, vote_decay=1.0, class_gate=1, motion=1)


def conf_keys(conf: np.ndarray) -> np.ndarray:
    """descending det_conf == descending key: the fp32 bit patterns ordered as signed magnitudes, never 0"""
    u = np.ascontiguousarray(conf, dtype=np.float32).view(np.uint32)
    k = np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000))
    return np.maximum(k, np.uint32(1))


def iou_det_tracks(box: np.ndarray, pred: np.ndarray) -> np.ndarray:
    """nms_suppressed's IoU expression with the detection `box` [4] as i and the predicted boxes `pred` [n, 4] as j, fp32"""
    ix1, iy1, ix2, iy2 = (F(v) for v in box)
    ai = F(F(ix2 - ix1) * F(iy2 - iy1))
    jx1, jy1, jx2, jy2 = pred[:, 0], pred[:, 1], pred[:, 2], pred[:, 3]
    aj = (jx2 - jx1) * (jy2 - jy1)
    with np.errstate(invalid="ignore"):
        w = np.maximum(F(0), np.minimum(ix2, jx2) - np.maximum(ix1, jx1))
        h = np.maximum(F(0), np.minimum(iy2, jy2) - np.maximum(iy1, jy1))
        inter = w * h
        return (inter / (((ai + aj) - inter) + EPS)).astype(np.float32)


class _Stream:
    def __init__(self, T: int, nc: int):
        self.box = np.zeros((T, 4), np.float32)
        self.vel = np.zeros((T, 4), np.float32)
        self.id = np.zeros(T, np.int32)
        self.hits = np.zeros(T, np.int32)
        self.missed = np.zeros(T, np.int32)
        self.age = np.zeros(T, np.int32)
        self.cls = np.zeros(T, np.int32)
        self.wsum = np.zeros(T, np.float32)
        self.vote = np.zeros(T, np.int32)
        self.live = np.zeros(T, bool)
        self.acc = np.zeros((T, nc), np.float32)
        self.next_id = 1
        self.overflow = 0


class TrackerRef:
    def __init__(self, max_det: int, num_classes: int = 58, **cfg):
        c = dict(DEFAULTS)
        for k, v in cfg.items():
            if k not in DEFAULTS:
                raise TypeError(f"unknown tracker setting {k!r}")
            c[k] = v
        self.cfg = c
        self.max_det, self.nc = int(max_det), max(int(num_classes), 1)
        self.T = int(c["max_tracks"])
        self.iou_match, self.new_conf, self.decay = F(c["iou_match"]), F(c["new_conf"]), F(c["vote_decay"])
        self.streams = [_Stream(self.T, self.nc) for _ in range(int(c["n_streams"]))]
        # smallest distance of a match decision from flipping: |IoU - iou_match| of every candidate, best - second best
        self.min_margin = float("inf")

    def reset(self, stream: int = -1) -> None:
        for s in (self.streams if stream < 0 else [self.streams[stream]]):
            s.live[:] = False

    # ---- one frame of one stream -----------------------------------------------------------------------------------------
    def _vote(self, st: _Stream, s: int, cls: int, conf) -> None:
        if 0 <= cls < self.nc:
            st.acc[s] = st.acc[s] * self.decay
            st.wsum[s] = F(F(st.wsum[s] * self.decay) + F(conf))
            st.acc[s, cls] = F(st.acc[s, cls] + F(conf))
            st.vote[s] = 1

    def _frame(self, st: _Stream, dets: np.ndarray, out: np.ndarray) -> None:
        c, n = self.cfg, len(dets)
        boxes = np.stack([dets["x1"], dets["y1"], dets["x2"], dets["y2"]], 1).astype(np.float32) if n else np.zeros((0, 4), np.float32)
        # 1 predict
        dt = (st.missed + 1).astype(np.float32)
        pred = (st.box + st.vel * dt[:, None]).astype(np.float32) if c["motion"] else st.box.copy()
        was_live = st.live.copy()
        claimed = np.zeros(self.T, bool)
        asg = np.full(n, -1, np.int64)
        # 2 match + 3 update
        keys = conf_keys(dets["det_conf"]) if n else np.zeros(0, np.uint32)
        order = sorted(range(n), key=lambda i: (-int(keys[i]), i))
        for d in order:
            cand = st.live & was_live & ~claimed
            if c["class_gate"]:
                cand &= st.cls == dets["det_class"][d]
            slots = np.flatnonzero(cand)
            if len(slots) == 0:
                continue
            iou = iou_det_tracks(boxes[d], pred[slots])
            with np.errstate(invalid="ignore"):
                ok = iou > self.iou_match
            fin = iou[~np.isnan(iou)]
            if len(fin):
                self.min_margin = min(self.min_margin, float(np.abs(fin.astype(np.float64) - float(self.iou_match)).min()))
            if not ok.any():
                continue
            good = np.sort(iou[ok].astype(np.float64))[::-1]
            if len(good) > 1:
                self.min_margin = min(self.min_margin, float(good[0] - good[1]))
            best = iou[ok].max()
            s = int(slots[ok & (iou == best)][0])   # ties: lower slot
            if c["motion"]:
                st.vel[s] = (boxes[d] - st.box[s]) / dt[s]
            st.box[s] = boxes[d]
            st.hits[s] += 1
            st.missed[s] = 0
            claimed[s] = True
            asg[d] = s
            self._vote(st, s, int(dets["cls_class"][d]), dets["cls_conf"][d])
        # 4 age
        lost = st.live & ~claimed
        st.missed[lost] += 1
        st.live[lost & (st.missed > c["max_age"])] = False
        st.age[st.live] += 1
        # 5 birth
        born = np.zeros(self.T, bool)
        free = list(np.flatnonzero(~st.live))
        for d in range(n):
            if asg[d] >= 0 or not (dets["det_conf"][d] >= self.new_conf):
                continue
            if not free:
                st.overflow += 1
                continue
            s = int(free.pop(0))
            st.box[s], st.vel[s] = boxes[d], 0
            st.id[s], st.next_id = st.next_id, st.next_id + 1
            st.hits[s], st.missed[s], st.age[s], st.cls[s] = 1, 0, 0, dets["det_class"][d]
            st.acc[s], st.wsum[s], st.vote[s] = 0, 0, 0
            st.live[s] = born[s] = True
            asg[d] = s
            self._vote(st, s, int(dets["cls_class"][d]), dets["cls_conf"][d])
        # 6 emit
        for d in range(n):
            s = int(asg[d])
            if s < 0:
                out[d] = (0, -1, 0, 0, -1, 0, 0, 0)
                continue
            vc = int(np.argmax(st.acc[s]))   # ties: lower class
            has = bool(st.vote[s])
            vconf = F(st.acc[s, vc] / st.wsum[s]) if has and st.wsum[s] > 0 else F(0)
            flags = (CONFIRMED if st.hits[s] >= c["min_hits"] else 0) | (BORN if born[s] else 0)
            out[d] = (st.id[s], s, st.hits[s], st.age[s], vc if has else -1, vconf, st.wsum[s], flags)

    # ---- the entry points ------------------------------------------------------------------------------------------------
    def track(self, dets: np.ndarray, counts, stream_ids=None) -> np.ndarray:
        d = np.asarray(dets, dtype=DET_DTYPE).reshape(-1, self.max_det)
        B = d.shape[0]
        out = np.zeros((B, self.max_det), dtype=TRACK_DTYPE)
        for b in range(B):   # the frames of one stream in batch order; streams do not interact
            n = min(max(int(counts[b]), 0), self.max_det)
            self._frame(self.streams[0 if stream_ids is None else int(stream_ids[b])], d[b, :n], out[b])
        return out

    def snapshot(self, stream: int = 0) -> dict:
        st = self.streams[stream]
        slots = np.flatnonzero(st.live)
        t = np.zeros(len(slots), dtype=TRACK_STATE_DTYPE)
        t["slot"], t["track_id"] = slots, st.id[slots]
        for k, f in enumerate(("x1", "y1", "x2", "y2")):
            t[f], t["v" + f] = st.box[slots, k], st.vel[slots, k]
        t["hits"], t["missed"], t["age"], t["det_class"] = st.hits[slots], st.missed[slots], st.age[slots], st.cls[slots]
        t["wsum"], t["has_vote"] = st.wsum[slots], st.vote[slots]
        return {"tracks": t, "acc": st.acc[slots].copy(), "next_id": st.next_id, "overflow": st.overflow}


# ---- scenes -----------------------------------------------------------------------------------------------------------------
def make_scene(seed: int, max_det: int, num_classes: int = 58, n_frames=None, n_signs=None, frame_hw=(270, 480)):
    """A synthetic record stream: (dets [n_frames, max_det], counts [n_frames]).  n_frames (40..200) and the number of signs in
    the scene's life (1..30) are drawn from the seed unless given.  Signs are born and die, drift with a constant velocity,
    grow, jitter by up to a pixel, and are dropped for single frames or short gaps; the classifier label is the sign's true
    class 70 % of the time, another class otherwise, and some records carry cls_class = -1.  Record order within a frame is
    shuffled.  At most max_det records per frame (the lowest-scored ones are cut, as the pipeline's max_det does)."""
    rng = np.random.default_rng(seed)
    n_frames = int(rng.integers(40, 201)) if n_frames is None else int(n_frames)
    n_signs = int(rng.integers(1, 31)) if n_signs is None else int(n_signs)
    H, W = frame_hw
    signs = []
    for _ in range(n_signs):
        t0 = int(rng.integers(0, max(1, n_frames - 10)))
        life = int(rng.integers(8, 80))
        size = float(rng.uniform(14, 70))
        signs.append(dict(t0=t0, t1=min(n_frames, t0 + life), cx=float(rng.uniform(60, W - 60)), cy=float(rng.uniform(60, H - 60)),
                          vx=float(rng.uniform(-6, 6)), vy=float(rng.uniform(-3, 3)), size=size, grow=float(rng.uniform(1.0, 1.03)),
                          aspect=float(rng.uniform(0.8, 1.25)), det_class=int(rng.integers(0, 3)), true_cls=int(rng.integers(0, num_classes)),
                          p_drop=float(rng.choice([0.0, 0.1, 0.3])), gap_at=int(rng.integers(t0 + 2, t0 + life + 2)), gap_len=int(rng.integers(1, 6))))
    dets = np.zeros((n_frames, max_det), dtype=DET_DTYPE)
    counts = np.zeros(n_frames, np.int32)
    for t in range(n_frames):
        recs = []
        for s in signs:
            if not (s["t0"] <= t < s["t1"]):
                continue
            if rng.random() < s["p_drop"] or s["gap_at"] <= t < s["gap_at"] + s["gap_len"]:
                continue
            k = t - s["t0"]
            cx, cy = s["cx"] + s["vx"] * k + rng.uniform(-1, 1), s["cy"] + s["vy"] * k + rng.uniform(-1, 1)
            w = s["size"] * s["grow"] ** k + rng.uniform(-1, 1)
            h = w * s["aspect"] + rng.uniform(-1, 1)
            x1, y1, x2, y2 = max(cx - w / 2, 0.0), max(cy - h / 2, 0.0), min(cx + w / 2, float(W)), min(cy + h / 2, float(H))
            if x2 - x1 < 4 or y2 - y1 < 4:
                continue
            u = rng.random()
            if u < 0.08:
                cls, cconf = -1, 0.0
            elif u < 0.08 + 0.92 * 0.7:
                cls, cconf = s["true_cls"], float(rng.uniform(0.4, 1.0))
            else:
                cls, cconf = int((s["true_cls"] + rng.integers(1, num_classes)) % num_classes), float(rng.uniform(0.2, 0.7))
            recs.append((x1, y1, x2, y2, float(rng.uniform(0.25, 0.99)), s["det_class"], cls, cconf))
        if len(recs) > max_det:
            recs = sorted(recs, key=lambda r: -r[4])[:max_det]
        perm = rng.permutation(len(recs))
        for i, j in enumerate(perm):
            dets[t, i] = recs[j]
        counts[t] = len(recs)
    return dets, counts


def scene_margin(dets, counts, max_det: int, num_classes: int, **cfg) -> float:
    """the smallest decision margin of the oracle over a scene (the GPU tests assert it is at least 1e-4)"""
    ref = TrackerRef(max_det=max_det, num_classes=num_classes, **cfg)
    ref.track(dets, counts)
    return ref.min_margin
