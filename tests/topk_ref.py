"""NumPy restatement of the top-k rule and of the distribution vote of include/litepi.h (lp_topk, lp_track_topk) and the record
generators of their tests.  Nothing in the reference keeps more than the arg-max, so this file is what pins both.

    rec = select(p, k)                              # one TOPK_DTYPE record of the distribution p [nc]
    ref = TrackerTopkRef(max_det=16, num_classes=58, max_tracks=8)
    tracks = ref.track_topk(dets, counts, topk)     # the tracker's rule with every detection voting its lp_topk record
    tracks = ref.track(dets, counts)                # the vote on (cls_class, cls_conf), on the same accumulators
"""
from __future__ import annotations

import numpy as np

from tracking_ref import DET_DTYPE, TRACK_DTYPE, F, TrackerRef

TOPK_MAX = 8
TOPK_DTYPE = [("cls", "<i4", (TOPK_MAX,)), ("prob", "<f4", (TOPK_MAX,))]


def empty_records(shape) -> np.ndarray:
    """records of no classes: every cls = -1, every prob = 0"""
    t = np.zeros(shape, dtype=TOPK_DTYPE)
    t["cls"] = -1
    return t


def select(p, k: int) -> np.ndarray:
    """The selection rule: the classes ordered by p descending, ties by class ascending; the first min(k, nc) with their p
    unchanged, the other entries cls = -1, prob = 0."""
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1)
    order = np.argsort(-p.astype(np.float64), kind="stable")   # stable: equal values keep ascending class order
    m = min(int(k), len(p))
    rec = empty_records(1)[0]
    rec["cls"][:m] = order[:m]
    rec["prob"][:m] = p[order[:m]]
    return rec


def is_empty(t: np.ndarray) -> np.ndarray:
    return (t["cls"] == -1).all(-1) & (t["prob"].view(np.uint32) == 0).all(-1)


# ---- distributions of the selection tests --------------------------------------------------------------------------------
def distributions(nc: int, seed: int = 0) -> dict:
    """name -> p [nc] float32: softmax of random logits, all equal, one-hot (the zero ties come out lowest class first),
    ascending and descending ramps, and one whose winners are class nc - 1 and class 64 (when it exists)"""
    rng = np.random.default_rng(1000 * nc + seed)
    z = rng.normal(0, 3, nc)
    e = np.exp(z - z.max())
    hot = np.zeros(nc, np.float32)
    hot[int(rng.integers(0, nc))] = 1.0
    ramp = (np.arange(1, nc + 1, dtype=np.float64) / (nc * (nc + 1) / 2)).astype(np.float32)
    ends = np.full(nc, 0.1 / nc, np.float32)
    ends[nc - 1] = 0.5
    if nc > 64:
        ends[64] = 0.4
    return {"softmax": (e / e.sum()).astype(np.float32), "equal": np.full(nc, 1.0 / nc, np.float32), "one_hot": hot,
            "ascending": ramp, "descending": ramp[::-1].copy(), "last_and_64": ends}


# ---- records of the tracker tests ---------------------------------------------------------------------------------------
def one_entry_records(dets: np.ndarray, num_classes: int) -> np.ndarray:
    """lp_topk records that say what the lp_det fields say: (cls_class, cls_conf) as the only entry of a classified detection"""
    d = np.asarray(dets, dtype=DET_DTYPE)
    t = empty_records(d.shape)
    ok = (d["cls_class"] >= 0) & (d["cls_class"] < num_classes)
    t["cls"][..., 0] = np.where(ok, d["cls_class"], -1)
    t["prob"][..., 0] = np.where(ok, d["cls_conf"], np.float32(0))
    return t


def random_records(seed: int, shape, num_classes: int, k: int, p_empty: float = 0.08) -> np.ndarray:
    """records holding a random k-entry head of a distribution: min(k, num_classes) distinct classes with descending
    probabilities that sum to at most 1; a share of p_empty of them empty (an unclassified detection)"""
    rng = np.random.default_rng(seed)
    t = empty_records(shape)
    m = min(int(k), int(num_classes))
    flat = t.reshape(-1)
    for r in flat:
        if rng.random() < p_empty:
            continue
        z = rng.normal(0, 2, num_classes)
        p = np.exp(z - z.max())
        p = (p / p.sum()).astype(np.float32)
        s = select(p, m)
        r["cls"], r["prob"] = s["cls"], s["prob"]
    return t


class TrackerTopkRef(TrackerRef):
    """TrackerRef with the distribution vote of lp_track_topk.  track_topk hands the base class's frame walk records whose
    cls_class field carries the record's INDEX in its frame, so _vote receives that index where the base passes cls_class
    and looks the lp_topk record up; track() is the base's vote on (cls_class, cls_conf).  Both work on the same accumulators."""

    _frame_topk = None

    def _vote(self, st, s: int, cls: int, conf) -> None:
        if self._frame_topk is None:
            return super()._vote(st, s, cls, conf)
        t = self._frame_topk[cls]   # cls: the record index
        tc, tp = t["cls"], t["prob"]
        if not 0 <= int(tc[0]) < self.nc:
            return
        valid = [j for j in range(TOPK_MAX) if 0 <= int(tc[j]) < self.nc]
        st.acc[s] = st.acc[s] * self.decay
        w = F(0)
        for j in valid:
            w = F(w + F(tp[j]))
        st.wsum[s] = F(F(st.wsum[s] * self.decay) + w)
        for j in valid:   # a class named twice is added twice, in j order
            st.acc[s, int(tc[j])] = F(st.acc[s, int(tc[j])] + F(tp[j]))
        st.vote[s] = 1

    def track_topk(self, dets: np.ndarray, counts, topk: np.ndarray, stream_ids=None) -> np.ndarray:
        d = np.array(np.asarray(dets, dtype=DET_DTYPE).reshape(-1, self.max_det))   # a copy: cls_class becomes the record index
        t = np.asarray(topk, dtype=TOPK_DTYPE).reshape(-1, self.max_det)
        B = d.shape[0]
        assert t.shape[0] == B
        d["cls_class"] = np.arange(self.max_det, dtype=np.int32)[None, :]
        out = np.zeros((B, self.max_det), dtype=TRACK_DTYPE)
        try:
            for b in range(B):
                n = min(max(int(counts[b]), 0), self.max_det)
                self._frame_topk = t[b]
                self._frame(self.streams[0 if stream_ids is None else int(stream_ids[b])], d[b, :n], out[b])
        finally:
            self._frame_topk = None
        return out


def acd_against_b(max_det: int, classes=(3, 7, 11, 20)):
    """The issue's example: one sign seen three times, (A .40, B .35), (C .40, B .35), (D .40, B .35).  Returns
    (dets [3, max_det], counts [3], topk [3, max_det], A, B): the top-1 vote says A at 0.40 of 1.20, the distribution says B."""
    A, Bc, Cc, Dc = classes
    dets = np.zeros((3, max_det), dtype=DET_DTYPE)
    topk = empty_records((3, max_det))
    for f, first in enumerate((A, Cc, Dc)):
        dets[f, 0] = (100.0, 80.0, 140.0, 120.0, 0.9, 0, first, 0.40)
        topk[f, 0]["cls"][:2] = (first, Bc)
        topk[f, 0]["prob"][:2] = (0.40, 0.35)
    return dets, np.ones(3, np.int32), topk, A, Bc
