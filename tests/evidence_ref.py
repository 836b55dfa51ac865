"""NumPy restatement of the evidence store's rule (include/litepi.h, lp_evidence_config): per inventory entry an E x E BGR
picture of the best sighting's surroundings and that picture's window.  The window arithmetic is fp32 with every operation
written out on its own; the picture is ``views_ref.make_view`` of the window.  Nothing here imports from the product.

    ref = EvidenceRef(max_det=8, track_cfg=dict(max_tracks=8, max_age=1), ev_cfg=dict(size=64, scale=2.0))
    ref.feed(dets, tracks, counts, frames=frames)            # frames [B, H, W, 3] BGR: crops = 1; frames=None: crops = 0
    signs, crops, pictures, windows, dropped = ref.drain_evidence()
"""
from __future__ import annotations

import math

import numpy as np

import inventory_ref as V
import views_ref

F = np.float32
HAS_EVIDENCE = 4
SIDE_MIN, SIDE_MAX = 16, 16384
EV_DEFAULTS = dict(size=128, scale=2.0)


def _fmax(a, b):
    """fmaxf: the non-NaN operand"""
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    return a if a > b else b


def _fmin(a, b):
    if np.isnan(a):
        return b
    if np.isnan(b):
        return a
    return a if a < b else b


def _centre(a, b, L: int) -> int:
    with np.errstate(invalid="ignore", over="ignore"):
        m = F(F(F(a) + F(b)) * F(0.5))
    return int(_fmin(_fmax(F(np.floor(m)), F(0)), F(L)))


def window(scale, H: int, W: int, box):
    """((x, y, w, h), has) of box (x1, y1, x2, y2) on an H x W frame; a zero window without a picture"""
    x1, y1, x2, y2 = (F(v) for v in box)
    with np.errstate(invalid="ignore", over="ignore"):
        bw, bh = F(x2 - x1), F(y2 - y1)
        if not (H >= 16 and W >= 16 and bool(bw > 0) and bool(bh > 0)):
            return (0, 0, 0, 0), False
        want = F(F(scale) * _fmax(bw, bh))
        side = int(_fmin(_fmax(F(np.ceil(want)), F(SIDE_MIN)), F(SIDE_MAX)))
    w, h = min(side, W), min(side, H)
    cx, cy = _centre(x1, x2, W), _centre(y1, y2, H)
    return (min(max(cx - w // 2, 0), W - w), min(max(cy - h // 2, 0), H - h), w, h), True


def picture(frame: np.ndarray, E: int, win) -> np.ndarray:
    return views_ref.make_view(frame, E, tuple(int(v) for v in win))[0]


class EvidenceRef(V.InventoryRef):
    def __init__(self, max_det: int, track_cfg=None, inv_cfg=None, crop_size: int = 64, ev_cfg=None):
        super().__init__(max_det, track_cfg, inv_cfg, crop_size)
        c = dict(EV_DEFAULTS)
        for k, v in (ev_cfg or {}).items():
            if k not in EV_DEFAULTS:
                raise TypeError(f"unknown evidence setting {k!r}")
            c[k] = v
        self.E, self.scale = int(c["size"]), F(c["scale"])
        self.ev = {}        # open entry (by identity) -> (picture, window)
        self.ev_log = []    # parallel to self.log
        self.rendered = 0   # pictures made: the device renders only final bests, the reference every best

    def _log_block(self, stream: int, slots, extra_flags: int) -> None:
        block = [self.entries[stream][s] for s in sorted(slots) if self.entries[stream][s].sign["hits"] >= self.min_hits]
        closing = [self.entries[stream][s] for s in slots]
        before = len(self.log)
        super()._log_block(stream, slots, extra_flags)
        for e in block[:len(self.log) - before]:
            self.ev_log.append(self.ev[id(e)] if e.sign["flags"] & HAS_EVIDENCE else None)
        for e in closing:
            self.ev.pop(id(e), None)

    def _frame(self, stream: int, dets, tracks, crop_of, frame=None) -> None:
        took = []

        def spy(i):
            took.append(i)
            return crop_of(i)
        super()._frame(stream, dets, tracks, spy)
        for i in took:   # the sightings that became their entry's best in this frame, after the rule's own step 4
            e = self.entries[stream][int(tracks["slot"][i])]
            e.sign["flags"] &= ~HAS_EVIDENCE
            self.ev.pop(id(e), None)
            if frame is None:
                continue
            win, has = window(self.scale, frame.shape[0], frame.shape[1], [dets[k][i] for k in ("x1", "y1", "x2", "y2")])
            if has:
                e.sign["flags"] |= HAS_EVIDENCE
                self.ev[id(e)] = (picture(frame, self.E, win), win)
                self.rendered += 1

    def feed(self, dets, tracks, counts, stream_ids=None, crops=None, has_crop=None, frames=None) -> None:
        """frames: None (crops = 0 for the call) or the call's [B] BGR frames; crops / has_crop as InventoryRef.feed"""
        d = np.asarray(dets, dtype=V.R.DET_DTYPE).reshape(-1, self.max_det)
        tr = np.asarray(tracks, dtype=V.R.TRACK_DTYPE).reshape(-1, self.max_det)
        for b in range(d.shape[0]):
            n = min(max(int(counts[b]), 0), self.max_det)

            def crop_of(i, b=b):
                if crops is None or frames is None:
                    return None
                if isinstance(crops, dict):
                    return crops.get((b, i))
                return crops[b][i] if has_crop is None or has_crop[b][i] else None
            self._frame(0 if stream_ids is None else int(stream_ids[b]), d[b, :n], tr[b, :n], crop_of, None if frames is None else frames[b])

    def drain_evidence(self):
        n = len(self.log)
        pics, wins = np.zeros((n, self.E, self.E, 3), np.uint8), np.zeros((n, 4), np.int32)
        for k, pw in enumerate(self.ev_log):
            if pw is not None:
                pics[k], wins[k] = pw
        self.ev_log = []
        signs, crops, dropped = self.drain()
        return signs, crops, pics, wins, dropped

    def drain(self):
        self.ev_log = []
        return super().drain()

    def open_evidence(self, stream: int = 0):
        ents = [e for e in self.entries[stream] if e is not None]
        pics, wins = np.zeros((len(ents), self.E, self.E, 3), np.uint8), np.zeros((len(ents), 4), np.int32)
        for k, e in enumerate(ents):
            if e.sign["flags"] & HAS_EVIDENCE:
                pics[k], wins[k] = self.ev[id(e)]
        return pics, wins
