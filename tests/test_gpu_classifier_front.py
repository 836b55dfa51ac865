"""cls_front's shared LDS regions (``-m gpu``).  cls_front runs one ROI per workgroup pass on a grid of min(capacity, 512)
workgroups, so past 512 ROIs a workgroup runs several ROIs in a row and every buffer of the second ROI lies where a buffer
of the first one was (IN / POOL / T2, STEM / T1 / D1 / stage 3.0's buffers, STEM's tail / X2, and stage 3.0's depthwise
parameters staged per ROI into the regions' tails).  Anything left over from the ROI before -- X2's padding channels, IN's
guards, a parameter set written too early -- would make a ROI's result depend on its predecessor.  No kernel reduces across
ROIs, so every slot must be bit-equal to the same pool ROI's result in the handle's 64-ROI baseline call, where each
workgroup runs one ROI.  Inputs, float64 reference and bound are those of tests/test_gpu_classifier.py."""
import numpy as np
import pytest

import test_gpu_classifier as T

pytestmark = pytest.mark.gpu

# (capacity, R): 3 workgroups / every workgroup but one / every workgroup run a second ROI; 1537 = 3 x 512 + 1: workgroup 0
# runs four ROIs, the others three
FRONT_CASES = [(515, 515), (1023, 1023), (1537, 1537)]


@pytest.mark.parametrize("cap,R", FRONT_CASES, ids=[f"{c}-{r}" for c, r in FRONT_CASES])
def test_several_rois_per_workgroup(cap, R):
    calls, _, _ = T._count_calls(cap, R)
    res = T._run("A", T._job("A", 91, cap, calls))
    T._check_names("A", res)
    T._check_counts("path A front", res, cap, R, T._ref(91), T._bound(91, "A"))


def _edge(name):
    """index of an edge crop in classifier_pool.pool(): 15 real crops, then 1x1, 1x300, 300x1, 64x64, all 0, all 255, 4096x3"""
    return 15 + ["1x1", "1x300", "300x1", "64x64", "zeros", "ones", "4096x3"].index(name)


@pytest.mark.parametrize("fixed", ["zeros", "ones", "64x64"])
@pytest.mark.parametrize("order", ["behind", "ahead"])
def test_every_pool_roi_next_to_a_fixed_one(fixed, order):
    """1024 slots on 512 workgroups: workgroup b runs slot b, then slot b + 512.  One half holds the same crop 512 times (all
    0, all 255, or the 64x64 crop whose resize is the identity), the other half every pool ROI eight times, so each pool ROI
    runs behind (or ahead of) the fixed crop in the same workgroup.  Every slot bit-equal to the pool baseline."""
    k = _edge(fixed)
    same, each = np.full(512, k), np.tile(np.arange(64), 8)
    idx = np.concatenate([same, each] if order == "behind" else [each, same])
    res = T._run("A", T._job("A", 91, 1024, [np.arange(64), idx]))
    T._check_names("A", res)
    base_ids, base_p = res["ids"][0], res["probs"][0]
    T._check_vs_ref(f"path A front {fixed} {order} pool", base_p, base_ids, T._ref(91), T._bound(91, "A"))
    ids, probs = res["ids"][1], res["probs"][1]
    ok = T._bits_equal(probs, base_p[idx]).all(axis=1) & (ids == base_ids[idx])
    print(f"CLS front {fixed} {order}: {int(ok.sum())} of 1024 slots bit-equal to the handle's baseline")
    assert ok.all(), f"{int((~ok).sum())} slots differ, first {np.flatnonzero(~ok)[:8].tolist()}"
