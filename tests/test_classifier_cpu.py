"""CPU checks of the ShuffleNetV2 classifier oracle and of the input conditions tests/test_gpu_classifier.py relies on:
the BN-folded float64 forward equals the float64 module, the argmax excuse stays rare under every path's bound, and the
seeded index sequences of the ROI-count cases repeat rarely at the offsets a mis-indexed pass would read."""
import functools

import numpy as np
import pytest
import torch

import classifier_pool as CP
from oracle import shufflenet_ref as S

# class counts each path is run with on the pool (tests/test_gpu_classifier.py)
FP16_COUNTS = {"fused": (2, 58, 64, 65, 91, 129, 560), "layerwise": (91, 256), "naive": (2, 91, 600)}
FP32_COUNTS = (2, 91, 600)


@functools.lru_cache(maxsize=None)
def _pool():
    return CP.pool()


@functools.lru_cache(maxsize=None)
def _ref(nc):
    sd = S.seeded_state_dict(nc)
    return sd, S.logp_module(S.build(nc, sd), S.input_batch(_pool()))


def _excuse_share(ref, bound):
    top2 = np.sort(ref, axis=1)[:, -2:]
    return float(np.mean(top2[:, 1] - top2[:, 0] < 2 * bound))


def test_pool_shape():
    rois = _pool()
    assert len(rois) == 64 and all(r.dtype == np.uint8 and r.ndim == 3 and r.shape[2] == 3 for r in rois)
    shapes = [r.shape[:2] for r in rois[15:22]]
    assert shapes == [(1, 1), (1, 300), (300, 1), (64, 64), (40, 50), (40, 50), (4096, 3)]
    assert not rois[19].any() and (rois[20] == 255).all()


@pytest.mark.parametrize("nc", [2, 91, 600])
def test_folded_forward_equals_float64_module(nc):
    """BN folded as classifier.cpp does, no rounding: the float64 module to 1e-9 in log p on the pool."""
    sd, ref = _ref(nc)
    err = np.abs(S.folded_logp(sd, _pool()) - ref).max()
    print(f"{nc} classes: folded vs module {err:.2e}")
    assert err <= 1e-9


@pytest.mark.parametrize("recipe", list(S.RECIPES))
def test_fp16_emulation_rounds_something(recipe):
    """Each recipe moves log p by far more than the float64 noise and far less than the old 3e-2 probability bound would
    allow in log p; its error is what the GPU bounds are built from."""
    sd, ref = _ref(91)
    err = np.abs(S.folded_logp(sd, _pool(), recipe) - ref)
    print(f"{recipe}: emulation max {err.max():.2e} mean {err.mean():.2e}")
    assert 1e-4 < err.max() < 5e-2 and err.mean() > 1e-5


@pytest.mark.parametrize("recipe,nc", [(r, n) for r, ns in FP16_COUNTS.items() for n in ns])
def test_argmax_excuses_are_rare_fp16(recipe, nc):
    """Share of pool ROIs whose float64 top-2 log-p margin is below 2 x bound (bound = 2 x the path's emulation max): <= 20 %."""
    sd, ref = _ref(nc)
    bound = 2 * np.abs(S.folded_logp(sd, _pool(), recipe) - ref).max()
    share = _excuse_share(ref, bound)
    print(f"{recipe} {nc}: bound {bound:.2e}, excused share {share:.3f}")
    assert share <= 0.20


@pytest.mark.parametrize("nc", FP32_COUNTS)
def test_argmax_excuses_are_rare_fp32(nc):
    """Same condition under the fp32 bound (10 x the float32-vs-float64 gap of the torch module)."""
    sd, ref = _ref(nc)
    bound = 10 * np.abs(S.logp_module(S.build(nc, sd), S.input_batch(_pool()), torch.float32) - ref).max()
    share = _excuse_share(ref, bound)
    print(f"fp32 {nc}: bound {bound:.2e}, excused share {share:.3f}")
    assert share <= 0.20


def test_index_sequences_rarely_repeat_at_pass_offsets():
    """For every (capacity, R) case: the share of slots i with pool[i] == pool[i + offset] is <= 5 % at the offsets 1 .. 2048
    (i.i.d. draws from 64 give 1.6 %), so a pass that reads ROIs at a wrong offset cannot hide behind repeated content."""
    for cap, R in sorted(set(CP.A_CASES + CP.OTHER_CASES)):
        idx = CP.draw(cap, R)
        assert idx.min() >= 0 and idx.max() < 64 and len(idx) == R
        for off, share in CP.repeat_shares(idx).items():
            assert share <= 0.05, f"case ({cap}, {R}), offset {off}: {share:.3f}"


@pytest.mark.parametrize("pair", CP.TIE_PAIRS)
def test_tie_weights_make_the_pair_top_two(pair):
    sd, ref = _ref(91)
    tsd = CP.tie_state_dict(sd, pair, ref)
    lp = S.logp_module(S.build(91, tsd), S.input_batch(_pool()))
    lo, hi = pair
    assert torch.equal(tsd["fc.weight"][lo], tsd["fc.weight"][hi]) and float(tsd["fc.bias"][lo]) == float(tsd["fc.bias"][hi])
    top2 = np.sort(np.argsort(-lp, axis=1)[:, :2], axis=1)
    assert (top2 == np.array(pair)).all()
    assert (np.delete(lp, [lo, hi], axis=1).max(axis=1) <= lp[:, lo] - 1.0).all()
    assert lp.min() > -60.0   # no fp32 probability underflows on the GPU
