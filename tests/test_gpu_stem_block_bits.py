"""stem_block_kernel / stem_block16_kernel (the network head in one launch) against a recording of the commit before their staging
and walk were rewritten (row-wise staging with the row arithmetic on the scalar unit, csrc/stem_walk.h's incremental offsets).

That rewrite changes addressing only: the same MFMAs with the same operands in the same order, the same K-group order, SiLU form
and fp16 rounding points.  So detect_raw's out0 must be what the parent commit produced, byte for byte.  tests/golden/
stem_block_out0.npz was written by tools/make_stem_goldens.py ON THE PARENT COMMIT; it holds, per case, the SHA-256 of out0's
bytes, the first launch's name and 64 sampled values.  Cases (seeded weights and images as test_gpu_parity.
test_stem_block16_equals_unfused_plan_v2), for v1 and v2:

* 352 x 352, batch 2: 88 = 2.75 x 32 output columns, 11 x 8 rows: border and partial tiles;
* 640 x 640, batch 1: the interior and the border form of the stem loop;
* det_input_h = 384 at width 640, batch 1: the fused head launch IS planned there (recorded, and asserted below).
"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location("make_stem_goldens", os.path.join(ROOT, "tools", "make_stem_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def golden():
    with np.load(REC.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_holds_every_case(golden):
    assert len(REC.CASES) == 6
    for name, preset, hw, batch in REC.CASES:
        for f in ("sha256", "shape", "dtype", "first", "idx", "val"):
            assert f"{name}_{f}" in golden, (name, f)
        assert len(str(golden[name + "_sha256"])) == 64 and golden[name + "_idx"].shape == (REC.NSAMPLE,)
        # the fused head launch is planned in every case, the rectangular 384 x 640 input included
        assert str(golden[name + "_first"]) == ("stem_block16_f16" if preset == "v2" else "stem_block_f16"), name


@pytest.mark.parametrize("name,preset,hw,batch", REC.CASES, ids=[c[0] for c in REC.CASES])
def test_out0_is_the_parents_byte_for_byte(tmp_path, golden, name, preset, hw, batch):
    out0, names = REC.run_case(preset, hw, batch, str(tmp_path))
    want_first = "stem_block16_f16" if preset == "v2" else "stem_block_f16"
    assert names[0] == want_first == str(golden[name + "_first"]), names[:3]
    assert list(out0.shape) == list(golden[name + "_shape"]) and str(out0.dtype) == str(golden[name + "_dtype"])
    idx, val = golden[name + "_idx"], golden[name + "_val"]
    assert np.array_equal(idx, REC.sample_index(out0.size))
    got = out0.ravel()[idx]
    bad = np.nonzero(got.view(np.uint32) != val.view(np.uint32))[0]
    assert bad.size == 0, (f"{name}: {bad.size} of {REC.NSAMPLE} sampled values differ from the parent's, e.g. flat index {int(idx[bad[0]])}: "
                           f"{got[bad[0]]!r} != {val[bad[0]]!r} (max |diff| over the samples {np.abs(got - val).max():.3g})")
    assert REC.digest(out0) == str(golden[name + "_sha256"]), f"{name}: the 64 samples agree, out0's SHA-256 does not"
