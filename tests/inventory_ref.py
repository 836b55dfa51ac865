"""NumPy restatement of the sign inventory's rule (include/litepi.h, lp_inventory_config): one record and best crop per finished
track, built from the lp_det / lp_track records of each frame alone.  Every fp32 operation is written out on its own, so the
device result must be bit-equal.

    ref = InventoryRef(max_det=16, track_cfg=dict(max_tracks=8, max_age=3), inv_cfg=dict(best=BEST_AREA))
    ref.feed(dets, tracks, counts)             # [B, max_det] lp_det and lp_track records, [B] counts
    signs, crops, dropped = ref.drain()        # SIGN_DTYPE records, [n, S, S, 3] uint8, signs lost to a full log
"""
from __future__ import annotations

import numpy as np

import tracking_ref as R

SIGN_DTYPE = [("stream", "<i4"), ("track_id", "<i4"), ("first_frame", "<i4"), ("last_frame", "<i4"), ("hits", "<i4"), ("voted_class", "<i4"),
              ("voted_conf", "<f4"), ("vote_weight", "<f4"), ("best_frame", "<i4"), ("best_quality", "<f4"), ("x1", "<f4"), ("y1", "<f4"),
              ("x2", "<f4"), ("y2", "<f4"), ("det_class", "<i4"), ("flags", "<i4")]
BEST_AREA, BEST_DET_CONF, BEST_CLS_CONF = 0, 1, 2
HAS_CROP, FLUSHED = 1, 2
F = np.float32

INV_DEFAULTS = dict(max_signs=4096, keep_crops=1, best=BEST_AREA, min_hits=0)


def quality(det, best: int):
    """the quality of a sighting, fp32, each operation rounded on its own"""
    if best == BEST_AREA:
        with np.errstate(invalid="ignore", over="ignore"):
            return F(F(F(det["x2"]) - F(det["x1"])) * F(F(det["y2"]) - F(det["y1"])))
    if best == BEST_DET_CONF:
        return F(det["det_conf"])
    return F(det["cls_conf"]) if int(det["cls_class"]) >= 0 else F(-1.0)


def rois_to_crops(crops, img, slot, total=None) -> dict:
    """a ROI list as the pipeline leaves it -> {(frame, record): crop}: the first `total` entries count"""
    n = len(img) if total is None else int(total)
    return {(int(img[r]), int(slot[r])): np.asarray(crops[r]) for r in range(n)}


class _Entry:
    __slots__ = ("sign", "missed", "crop")

    def __init__(self):
        self.sign, self.missed, self.crop = None, 0, None


class InventoryRef:
    def __init__(self, max_det: int, track_cfg=None, inv_cfg=None, crop_size: int = 64):
        t = dict(R.DEFAULTS)
        t.update(track_cfg or {})
        c = dict(INV_DEFAULTS)
        for k, v in (inv_cfg or {}).items():
            if k not in INV_DEFAULTS:
                raise TypeError(f"unknown inventory setting {k!r}")
            c[k] = v
        self.cfg = c
        self.max_det, self.T, self.max_age = int(max_det), int(t["max_tracks"]), int(t["max_age"])
        self.min_hits = int(c["min_hits"]) if int(c["min_hits"]) > 0 else int(t["min_hits"])
        self.best, self.max_signs, self.S = int(c["best"]), int(c["max_signs"]), int(crop_size)
        self.entries = [[None] * self.T for _ in range(int(t["n_streams"]))]
        self.frame_no = [0] * int(t["n_streams"])
        self.log, self.dropped = [], 0

    # ---- the log ---------------------------------------------------------------------------------------------------------
    def _log_block(self, stream: int, slots, extra_flags: int) -> None:
        """the closing entries of one (stream, frame) in ascending slot order; what does not fit is dropped"""
        block = [self.entries[stream][s] for s in sorted(slots) if self.entries[stream][s].sign["hits"] >= self.min_hits]
        for s in slots:
            self.entries[stream][s] = None
        room = max(self.max_signs - len(self.log), 0)
        for e in block[:room]:
            sign = e.sign.copy()
            sign["flags"] |= extra_flags
            self.log.append((sign, e.crop if sign["flags"] & HAS_CROP else None))
        self.dropped += len(block) - min(len(block), room)

    # ---- one frame of one stream ------------------------------------------------------------------------------------------
    def _frame(self, stream: int, dets, tracks, crop_of) -> None:
        t = self.frame_no[stream]
        ent = self.entries[stream]
        # 1 sight: the lowest record index that names a slot
        sight = {}
        for i in range(len(tracks)):
            s = int(tracks["slot"][i])
            if tracks["track_id"][i] > 0 and 0 <= s < self.T and s not in sight:
                sight[s] = i
        # 2 close
        closing = []
        for s in range(self.T):
            e = ent[s]
            if e is None:
                continue
            if s in sight:
                if int(tracks["track_id"][sight[s]]) != int(e.sign["track_id"]):
                    closing.append(s)
            elif e.missed + 1 > self.max_age:
                closing.append(s)
            else:
                e.missed += 1
        # 3 log
        if closing:
            self._log_block(stream, closing, 0)
        # 4 open / update
        for s, i in sorted(sight.items()):
            d, tr = dets[i], tracks[i]
            e = ent[s]
            opened = e is None
            if opened:
                e = ent[s] = _Entry()
                e.sign = np.zeros((), dtype=SIGN_DTYPE)
                e.sign["stream"], e.sign["track_id"], e.sign["first_frame"] = stream, tr["track_id"], t
            sg = e.sign
            sg["last_frame"], sg["hits"] = t, tr["hits"]
            sg["voted_class"], sg["voted_conf"], sg["vote_weight"] = tr["voted_class"], tr["voted_conf"], tr["vote_weight"]
            e.missed = 0
            q = quality(d, self.best)
            if opened or bool(q > sg["best_quality"]):   # false for a NaN
                sg["best_frame"], sg["best_quality"] = t, q
                sg["x1"], sg["y1"], sg["x2"], sg["y2"], sg["det_class"] = d["x1"], d["y1"], d["x2"], d["y2"], d["det_class"]
                crop = crop_of(i)
                e.crop = None if crop is None else np.array(crop, dtype=np.uint8).reshape(self.S, self.S, 3)
                sg["flags"] = HAS_CROP if crop is not None else 0
        # 5
        self.frame_no[stream] = t + 1

    # ---- the entry points -------------------------------------------------------------------------------------------------
    def feed(self, dets, tracks, counts, stream_ids=None, crops=None, has_crop=None) -> None:
        """crops: None (crops = 0), a dict {(frame, record): crop} or an array [B, max_det, S, S, 3]; has_crop [B, max_det]
        limits an array's crops (a dict's keys say which records have one)"""
        d = np.asarray(dets, dtype=R.DET_DTYPE).reshape(-1, self.max_det)
        tr = np.asarray(tracks, dtype=R.TRACK_DTYPE).reshape(-1, self.max_det)
        for b in range(d.shape[0]):
            n = min(max(int(counts[b]), 0), self.max_det)

            def crop_of(i, b=b):
                if crops is None:
                    return None
                if isinstance(crops, dict):
                    return crops.get((b, i))
                return crops[b][i] if has_crop is None or has_crop[b][i] else None
            self._frame(0 if stream_ids is None else int(stream_ids[b]), d[b, :n], tr[b, :n], crop_of)

    def flush(self, stream: int = -1) -> None:
        for st in (range(len(self.entries)) if stream < 0 else [stream]):
            slots = [s for s in range(self.T) if self.entries[st][s] is not None]
            if slots:
                self._log_block(st, slots, FLUSHED)

    def drain(self):
        signs = np.array([s for s, _ in self.log], dtype=SIGN_DTYPE).reshape(-1)
        crops = np.zeros((len(self.log), self.S, self.S, 3), np.uint8)
        for k, (_, c) in enumerate(self.log):
            if c is not None:
                crops[k] = c
        dropped, self.log, self.dropped = self.dropped, [], 0
        return signs, crops, dropped

    def open(self, stream: int = 0) -> np.ndarray:
        """the open entries of a stream in slot order, as they would be logged now"""
        return np.array([e.sign for e in self.entries[stream] if e is not None], dtype=SIGN_DTYPE).reshape(-1)

    def open_state(self, stream: int = 0):
        """(slot, track_id, missed) of the open entries, in slot order"""
        return [(s, int(e.sign["track_id"]), e.missed) for s, e in enumerate(self.entries[stream]) if e is not None]
