"""NumPy restatement of the crop quality rule (include/litepi.h, lp_quality): integer luma, 4-neighbour Laplacian on the interior,
int64 sums, the record in float64 with one conversion to float32 per field.  Every reduction is over integers, so the library's
records, host and device, must be bit-equal.  Also the inventory's rule under LP_RANK_SHARPNESS (InventorySharpRef) and the
seeded crops the tests share.

    rec = measure(crop)                       # [S, S, 3] uint8 RGB -> one QUALITY_DTYPE record
    recs = records_for(crops, img, slot, B, max_det)   # what a call over B frames leaves for a ROI list
"""
from __future__ import annotations

import numpy as np

import inventory_ref as I

QUALITY_DTYPE = [("sharpness", "<f4"), ("luma_mean", "<f4"), ("luma_var", "<f4"), ("clip_lo", "<f4"), ("clip_hi", "<f4"), ("flags", "<i4"),
                 ("reserved", "<i4", (2,))]
VALID = 1
RANK_CONFIG, RANK_SHARPNESS = 0, 1


def luma(crop) -> np.ndarray:
    c = np.asarray(crop, dtype=np.uint8).astype(np.int64)
    return (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8


def sums(crop) -> dict:
    Y = luma(crop)
    S = Y.shape[0]
    L = Y[:-2, 1:-1] + Y[2:, 1:-1] + Y[1:-1, :-2] + Y[1:-1, 2:] - 4 * Y[1:-1, 1:-1]
    return dict(n=(S - 2) * (S - 2), s1=int(L.sum()), s2=int((L * L).sum()), N=S * S, t1=int(Y.sum()), t2=int((Y * Y).sum()),
                lo=int((Y <= 4).sum()), hi=int((Y >= 251).sum()))


def measure(crop) -> np.ndarray:
    """the rule on one [S, S, 3] uint8 RGB crop.  The integer products are Python ints (exact); each float64 division is one
    correctly rounded operation."""
    s = sums(crop)
    D = np.float64
    n, N = D(s["n"]), D(s["N"])
    r = np.zeros((), dtype=QUALITY_DTYPE)
    r["sharpness"] = np.float32(D(s["n"] * s["s2"] - s["s1"] * s["s1"]) / (n * n))
    r["luma_mean"] = np.float32(D(s["t1"]) / N)
    r["luma_var"] = np.float32(D(s["N"] * s["t2"] - s["t1"] * s["t1"]) / (N * N))
    r["clip_lo"] = np.float32(D(s["lo"]) / N)
    r["clip_hi"] = np.float32(D(s["hi"]) / N)
    r["flags"] = VALID
    return r


def empty_records(shape) -> np.ndarray:
    r = np.zeros(shape, dtype=QUALITY_DTYPE)
    r["sharpness"] = -1.0
    return r


def is_empty(recs) -> np.ndarray:
    e = empty_records(())
    flat = np.ascontiguousarray(recs).reshape(-1)
    return np.array([x.tobytes() == e.tobytes() for x in flat]).reshape(np.shape(recs))


def records_for(crops, img, slot, B: int, max_det: int, before=None) -> np.ndarray:
    """the records a call over B frames leaves: empty everywhere, the measure at every (img[r], slot[r]) with img[r] < B; the
    records of frames >= B are those of `before` ([frames, max_det], default empty)"""
    out = empty_records((B, max_det)) if before is None else np.array(before, dtype=QUALITY_DTYPE)
    out[:B] = empty_records((B, max_det))
    for r in range(len(img)):
        if 0 <= img[r] < B and 0 <= slot[r] < max_det:
            out[img[r], slot[r]] = measure(crops[r])
    return out


# ---------------------------------------------------------------------------- the crops
def noise_crop(S: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(1000 * S + seed).integers(0, 256, (S, S, 3), dtype=np.uint8)


def sign_crop(S: int) -> np.ndarray:
    """a synthetic sign: a red ring around a white disc with a black bar, on a grey-blue ground"""
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    c = (S - 1) / 2.0
    rad = np.hypot(y - c, x - c)
    img = np.empty((S, S, 3), np.uint8)
    img[:] = (96, 120, 150)
    img[rad <= 0.45 * S] = (200, 30, 40)
    img[rad <= 0.33 * S] = (245, 245, 240)
    img[(np.abs(y - c) <= 0.07 * S) & (np.abs(x - c) <= 0.24 * S)] = (15, 15, 20)
    return img


def checkerboard_crop(S: int) -> np.ndarray:
    y, x = np.mgrid[0:S, 0:S]
    return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def box_blur(crop) -> np.ndarray:
    """3x3 box blur with replicated edges, rounded to nearest"""
    p = np.pad(np.asarray(crop, dtype=np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    S = crop.shape[0]
    acc = sum(p[dy:dy + S, dx:dx + S] for dy in range(3) for dx in range(3))
    return ((acc + 4) // 9).astype(np.uint8)


def extreme_crops(S: int) -> dict:
    return {"zeros": np.zeros((S, S, 3), np.uint8), "ones": np.full((S, S, 3), 255, np.uint8), "checkerboard": checkerboard_crop(S)}


def shared_crops(S: int) -> dict:
    """the crops the CPU and the GPU tests share, by name"""
    sign = sign_crop(S)
    out = {"noise0": noise_crop(S, 0), "noise1": noise_crop(S, 1), "sign": sign, "sign_blur": box_blur(sign), "sign_blur2": box_blur(box_blur(sign))}
    out.update(extreme_crops(S))
    return out


# ---------------------------------------------------------------------------- the inventory under LP_RANK_SHARPNESS
class InventorySharpRef(I.InventoryRef):
    """InventoryRef with step 4's q taken from the records' lp_quality: q = quality[b, i]["sharpness"] as it is (-1 for an empty
    record).  Only how q is obtained differs: the records reach the parent's rule with (cls_class, cls_conf) = (0, sharpness)
    under BEST_CLS_CONF, which reads exactly that pair for q.
    This DEPENDS on InventoryRef._frame reading lp_det's cls_class / cls_conf nowhere but in quality(): the sign takes its
    class from the lp_track record and copies only the box and det_class from lp_det.  Should the parent's rule ever copy
    either field into the sign, this substitution would show as a byte difference in the signs the tests compare, and q must
    then be passed in another way."""

    def feed(self, dets, tracks, counts, stream_ids=None, crops=None, has_crop=None, quality=None) -> None:
        if quality is None:   # LP_RANK_CONFIG
            return super().feed(dets, tracks, counts, stream_ids, crops, has_crop)
        d = np.array(dets, dtype=I.R.DET_DTYPE).reshape(-1, self.max_det)
        q = np.asarray(quality, dtype=QUALITY_DTYPE).reshape(-1, self.max_det)
        d["cls_class"], d["cls_conf"] = 0, q["sharpness"][:d.shape[0]]
        keep, self.best = self.best, I.BEST_CLS_CONF
        try:
            super().feed(d, tracks, counts, stream_ids, crops, has_crop)
        finally:
            self.best = keep
