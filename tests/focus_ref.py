"""NumPy float32 restatement of the focus rule of include/litepi.h (lp_focus_config): which windows a frame is seen through,
given the tracker's live tracks.  Every fp32 operation is written out on its own, in the header's order, so the device plan
must be equal int for int.

    ref = FocusRef(det_input=64, n_streams=2, motion=1, slots=3)
    views = ref.plan({0: snap0, 1: snap1}, heights, widths, stream_ids)   # [B, slots, 4] int32 {x, y, w, h}
    ref.state[0]                                                           # {"cursor": .., "unserved": ..}

A snapshot is an array of lp_track_state records (tracking_ref.TRACK_STATE_DTYPE: what Engine.tracker_snapshot and
TrackerRef.snapshot return under "tracks"), or anything with the fields slot, x1..y2, vx1..vy2, hits, missed.
"""
from __future__ import annotations

import math

import numpy as np

F = np.float32

DEFAULTS = dict(slots=3, side_min=0, side_max=0, margin=2.0, small_px=32.0, border=16, sweep=1, sweep_overlap=0)


def grid_axis(L: int, tile: int, overlap: int):
    """one axis of lp_view_grid: (origins, side)"""
    if L <= tile:
        return [0], L
    step = tile - overlap
    n = 1 + (L - tile + step - 1) // step
    return [min(k * step, L - tile) for k in range(n)], tile


def view_grid(tile: int, overlap: int, H: int, W: int):
    """the windows of lp_view_grid(tile, overlap, 0, H, W), row-major ([] when one window covers the frame)"""
    xs, sw = grid_axis(W, tile, overlap)
    ys, sh = grid_axis(H, tile, overlap)
    if len(xs) * len(ys) == 1:
        return []
    return [(x, y, sw, sh) for y in ys for x in xs]


def frame_ratio(det_input: int, H: int, W: int) -> np.float32:
    """the float ratio of the letterboxed whole frame (make_geom: the minimum of two double divisions, rounded to float)"""
    return F(min(det_input / H, det_input / W))


def covered(win, box, H: int, W: int, border: int) -> bool:
    x, y, w, h = win
    x1, y1, x2, y2 = box
    return bool((x == 0 or x1 >= F(x + border)) and (x + w == W or x2 <= F(x + w - border)) and
                (y == 0 or y1 >= F(y + border)) and (y + h == H or y2 <= F(y + h - border)))


class FocusRef:
    def __init__(self, det_input: int, n_streams: int = 1, motion: int = 1, **cfg):
        c = dict(DEFAULTS)
        for k, v in cfg.items():
            if k not in DEFAULTS:
                raise TypeError(f"unknown focus setting {k!r}")
            c[k] = v
        self.S = int(det_input)
        self.slots = int(c["slots"])
        self.side_min = int(c["side_min"]) or self.S
        self.side_max = int(c["side_max"]) or 2 * self.S
        self.margin, self.small_px = F(c["margin"]), F(c["small_px"])
        self.border, self.sweep, self.sweep_overlap = int(c["border"]), int(c["sweep"]), int(c["sweep_overlap"])
        self.motion = int(motion)
        self.state = [{"cursor": 0, "unserved": 0} for _ in range(int(n_streams))]

    # ---- step 1
    def askers(self, tracks, j: int, H: int, W: int):
        """[(slot, (x1, y1, x2, y2))] of the tracks that ask for a window in the j-th frame of their stream, in placement order"""
        rf = frame_ratio(self.S, H, W)
        out = []
        for t in tracks:
            dt = F(int(t["missed"]) + 1 + j)
            box = [F(t[k]) for k in ("x1", "y1", "x2", "y2")]
            vel = [F(t[k]) for k in ("vx1", "vy1", "vx2", "vy2")]
            with np.errstate(invalid="ignore", over="ignore"):
                p = [F(b + F(v * dt)) for b, v in zip(box, vel)] if self.motion else box
                if any(np.isnan(v) for v in p):
                    continue
                x1, y1 = max(p[0], F(0)), max(p[1], F(0))
                x2, y2 = min(p[2], F(W)), min(p[3], F(H))
                bw, bh = F(x2 - x1), F(y2 - y1)
                m = max(bw, bh)
                if bw > 0 and bh > 0 and F(m * rf) < self.small_px:
                    out.append((int(t["hits"]), int(t["slot"]), (x1, y1, x2, y2)))
        out.sort(key=lambda a: (-a[0], a[1]))
        return [(s, b) for _, s, b in out]

    # ---- steps 2 - 4 of one frame
    def frame(self, tracks, j: int, H: int, W: int, st: dict):
        placed = []
        for _, box in self.askers(tracks, j, H, W):
            if any(covered(w, box, H, W, self.border) for w in placed):
                continue
            if len(placed) >= self.slots:
                st["unserved"] += 1
                continue
            x1, y1, x2, y2 = box
            m = max(F(x2 - x1), F(y2 - y1))
            with np.errstate(over="ignore"):
                want = float(F(self.margin * m))
            side = self.side_max if want >= self.side_max else max(math.ceil(want), self.side_min)
            w, h = min(side, W), min(side, H)
            cx, cy = math.floor(float(F(F(x1 + x2) * F(0.5)))), math.floor(float(F(F(y1 + y2) * F(0.5))))
            placed.append((min(max(cx - w // 2, 0), W - w), min(max(cy - h // 2, 0), H - h), w, h))
        if self.sweep:
            G = view_grid(self.side_min, self.sweep_overlap, H, W)
            n = len(G)
            if n > 1:
                r = min(self.slots - len(placed), n)
                placed += [G[(st["cursor"] + i) % n] for i in range(r)]
                st["cursor"] = (st["cursor"] + r) % n
        return placed + [(0, 0, 0, 0)] * (self.slots - len(placed))

    def plan(self, tracks_by_stream, heights, widths, stream_ids=None, advance: bool = True) -> np.ndarray:
        B = len(heights)
        ids = [0] * B if stream_ids is None else [int(s) for s in stream_ids]
        out = np.zeros((B, self.slots, 4), np.int32)
        seen = {}
        work = {}
        for b in range(B):
            s = ids[b]
            st = work.setdefault(s, dict(self.state[s]))
            j = seen.get(s, 0)
            seen[s] = j + 1
            tracks = tracks_by_stream.get(s, []) if isinstance(tracks_by_stream, dict) else tracks_by_stream[s]
            out[b] = self.frame(tracks, j, int(heights[b]), int(widths[b]), st)
        if advance:
            for s, st in work.items():
                self.state[s] = st
        return out


def make_tracks(rows):
    """lp_track_state-like records from dicts / tuples (slot, x1, y1, x2, y2, vx1, vy1, vx2, vy2, hits, missed)"""
    dt = [("slot", "<i4"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("vx1", "<f4"), ("vy1", "<f4"), ("vx2", "<f4"),
          ("vy2", "<f4"), ("hits", "<i4"), ("missed", "<i4")]
    out = np.zeros(len(rows), dtype=dt)
    for i, r in enumerate(rows):
        if isinstance(r, dict):
            for k, v in r.items():
                out[i][k] = v
        else:
            out[i] = tuple(r)
    return out
