"""Shared inputs of the classifier tests (tests/test_gpu_classifier.py and tests/test_classifier_cpu.py): the 64-ROI pool, the seeded index sequences of the ROI-count cases, the tie-making weights,
and one runner that executes a list of classify calls on one handle.  Not a test module (no test_ prefix)."""
from __future__ import annotations

import io
import os
from typing import Dict, List, Sequence

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (capacity, R) of the ROI-count cases: path A takes all of them, paths B..E the last two of OTHER_CASES
A_CASES = [(1, 1), (4, 1), (4, 3), (5, 5), (64, 37), (512, 512), (600, 513), (1024, 1024), (1100, 1025), (2100, 2100), (4100, 4099)]
OTHER_CASES = [(64, 37), (1100, 1025)]
OFFSETS = (1, 4, 16, 64, 256, 512, 1024, 2048)
TIE_PAIRS = [(3, 40), (5, 69)]   # different lanes of the softmax wave / the same lane (69 = 5 + 64), at 91 classes


def _gen_rois(rng, n):
    """The generator of tests/test_gpu_parity.py::_rois (seeded noise crops 10..89 px a side), restated so that CPU tests
    need not import a GPU test module."""
    out = []
    for _ in range(n):
        h, w = int(rng.integers(10, 90)), int(rng.integers(10, 90))
        base = rng.integers(0, 256, (1, 1, 3))
        img = np.clip(base + rng.normal(0, 40, (h, w, 3)), 0, 255).astype(np.uint8)
        out.append(img)
    return out


def pool() -> List[np.ndarray]:
    """64 BGR uint8 crops: the 15 real sign crops of tests/golden/debug_rois.npz, 7 edge crops (1x1, 1x300, 300x1, 64x64
    -- the resize is the identity --, all 0, all 255, 4096x3; sizes are H x W), 42 crops of the _rois generator (seed 11:
    the first 37 are test_classifier_vs_oracle's)."""
    from PIL import Image
    with np.load(os.path.join(_ROOT, "tests", "golden", "debug_rois.npz")) as z:
        real = [np.asarray(Image.open(io.BytesIO(z[k].tobytes())).convert("RGB"))[..., ::-1].copy() for k in sorted(z.files)]
    rng = np.random.default_rng(5)
    edge = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((1, 1), (1, 300), (300, 1), (64, 64))]
    edge += [np.zeros((40, 50, 3), np.uint8), np.full((40, 50, 3), 255, np.uint8), rng.integers(0, 256, (4096, 3, 3), dtype=np.uint8)]
    out = real + edge + _gen_rois(np.random.default_rng(11), 42)
    assert len(out) == 64
    return [np.ascontiguousarray(r) for r in out]


def repeat_shares(idx: np.ndarray) -> Dict[int, float]:
    """Share of slots i with idx[i] == idx[i + offset], per offset (offsets past the sequence: no pairs, share 0)."""
    return {o: (float(np.mean(idx[:-o] == idx[o:])) if len(idx) > o else 0.0) for o in OFFSETS}


def draw(cap: int, R: int) -> np.ndarray:
    """Pool indices of the R slots of case (cap, R): i.i.d. uniform over the 64 pool ROIs, seeded by the case.  The first
    seed (cap, R, k), k = 0, 1, .., whose sequence repeats at no offset of OFFSETS in more than 5 % of the slots is taken
    (short sequences can repeat by chance: at R = 3 one equal neighbour is 50 %)."""
    for k in range(1000):
        idx = np.random.default_rng([cap, R, k]).integers(0, 64, R)
        if max(repeat_shares(idx).values()) <= 0.05:
            return idx
    raise AssertionError(f"no seed gives a rarely repeating sequence for ({cap}, {R})")


def tie_state_dict(sd, pair, ref_logp: np.ndarray):
    """sd with fc rows and biases of the two classes of ``pair`` identical, the pair's bias raised so that the two are the
    top two of every ROI by at least 2 in logit (ref_logp: float64 log p of ``sd`` on the ROIs, i.e. logits up to a per-ROI
    constant)."""
    lo, hi = pair
    out = {k: v.clone() for k, v in sd.items()}
    others = np.delete(ref_logp, [lo, hi], axis=1).max(axis=1)
    raise_by = float(np.max(others - ref_logp[:, lo])) + 2.0
    out["fc.weight"][hi] = out["fc.weight"][lo]
    b = float(out["fc.bias"][lo]) + max(raise_by, 0.0)
    out["fc.bias"][lo] = b
    out["fc.bias"][hi] = b
    return out


def run_job(job: dict, rois: Sequence[np.ndarray], monkeypatch=None) -> dict:
    """One handle: Engine(precision, max_batch=1, max_det=max_rois=cap), load job['sd'], then one classify call per entry of
    job['calls'] (pool indices; an entry longer than cap is classified in chunks of cap).  The first call is profiled.  A
    LitepiError at load or at any call ends the job: its text is returned under 'error'.  job['load_env'] (optional) is set in
    the environment around load_classifier alone, through pytest's monkeypatch."""
    from litepi import Engine, _ffi
    cap = job["cap"]
    res = {"ids": [], "probs": [], "names": [], "error": ""}
    e = Engine(precision=job["prec"], max_batch=1, max_det=cap, num_classes=job["nc"], max_rois=cap,
               conv_impl=job.get("impl", 0), cls_arch=job.get("arch", "shufflenetv2"))
    try:
        if job.get("load_env"):
            with monkeypatch.context() as m:
                for k, v in job["load_env"].items():
                    m.setenv(k, v)
                e.load_classifier(job["sd"])
        else:
            e.load_classifier(job["sd"])
        for n, call in enumerate(job["calls"]):
            ids, probs = [], []
            for c0 in range(0, len(call), cap):
                if n == 0 and c0 == 0:
                    e.profile_next(True)
                i, p = e.classify([rois[k] for k in call[c0:c0 + cap]])
                if n == 0 and c0 == 0:
                    res["names"] = sorted({k["name"] for k in e.profile_read()})
                ids.append(i)
                probs.append(p)
            res["ids"].append(np.concatenate(ids))
            res["probs"].append(np.concatenate(probs))
    except _ffi.LitepiError as ex:
        res["error"] = str(ex) or "LitepiError"
    finally:
        e.close()
    return res
