"""What lp_graph_stats counts behind every lp_run_* entry point (csrc/pipeline.cpp: run_or_capture, run_device_pass,
run_host_pass).

A key seen for the first time runs eagerly, the second call captures the step and launches the graph once, later calls replay
it.  A device entry point is one captured piece, a host entry point three (front, ROI resize, classifier).  So three identical
calls on a fresh handle show, cumulatively, (entries, eager, captures, replays) =

    device  (1, 1, 0, 0)  (1, 1, 1, 0)  (1, 1, 1, 1)
    host    (3, 3, 0, 0)  (3, 3, 3, 0)  (3, 3, 3, 3)

Then one call of ANOTHER entry point is made on the same handle: it must add entries of its own (run eagerly, capture and
replay nothing), and a fourth call of the first entry point must replay again without a new entry: no entry point replays
another's step, and none evicts it.

The other entry point is chosen so that it leaves the handle's geometry generation alone (a new view table, a new geometry or
a re-allocated frame buffer starts every captured step afresh, by design): it brings the same frames with the same geometry
and needs no buffer the first one has not sized.  Where the two take the same arguments -- the host pairs, whose keys name the
handle's own buffers, the device pairs on one frame batch, the two surfaces calls -- their keys differ in the entry point
alone.  Device batches under NV12 have sized the converted-frame buffer the host and surfaces calls use.

Models, frames and engine settings are tests/test_gpu_front_launches.py's (det_input 320, two frames of at most 400 x 500).
"""
import pytest

from test_gpu_front_launches import BIG, OVERLAP, SMALL, Call, make_engine, make_frames

pytestmark = pytest.mark.gpu

FULL = dict(views=["full"])
TILING = dict(overlap=OVERLAP, full_frame=True)


def _case(method, frames, fmt, **kw):
    return dict(method=method, frames=frames, fmt=fmt, kw=kw)


# (the entry point under test, pieces, the other entry point); "small": two SMALL frames, one view each under tiling
PAIRS = [
    (_case("run_batch", "big", "bgr"), 3, _case("run_batch_device", "big", "bgr")),
    (_case("run_batch_device", "big", "nv12"), 1, _case("run_surfaces_device", "big", "nv12")),
    (_case("run_tiled", "small", "bgr", **TILING), 3, _case("run_batch", "small", "bgr")),
    (_case("run_tiled_device", "small", "bgr", **TILING), 1, _case("run_batch_device", "small", "bgr")),
    (_case("run_views", "big", "bgr", **FULL), 3, _case("run_batch", "big", "bgr")),
    (_case("run_views_device", "big", "bgr", **FULL), 1, _case("run_batch_device", "big", "bgr")),
    (_case("run_focus", "big", "bgr"), 3, _case("run_focus_device", "big", "bgr")),
    (_case("run_focus_device", "big", "nv12"), 1, _case("run_focus", "big", "bgr")),
    (_case("run_surfaces_device", "big", "nv12"), 1, _case("run_batch_device", "big", "nv12")),
    (_case("run_views_surfaces_device", "big", "nv12", **FULL), 1, _case("run_surfaces_device", "big", "nv12")),
]
assert len({p[0]["method"] for p in PAIRS}) == 10


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import numpy as np
    import pixfmt_ref as R
    s = make_frames(tmp_path_factory.mktemp("graph_bookkeeping"))
    assert BIG[0] * BIG[1] * 3 % 16 == 0   # host uploads and converted frames sit where a packed device batch has them
    f0, f1 = s["models"]["frames"]
    small = [np.ascontiguousarray(f[:SMALL[0], :SMALL[1]]) for f in (f0, f1)]
    s["frames"]["bgr"]["small"] = small
    s["frames"]["nv12"]["small"] = [R.bgr_to_nv12(f) for f in small]
    return s


def _stats(e):
    s = e.graph_stats()
    return (s["entries"], s["eager"], s["captures"], s["replays"])


@pytest.mark.parametrize("first, n, other", PAIRS, ids=[p[0]["method"] for p in PAIRS])
def test_three_calls_then_another_entry_point(setup, first, n, other):
    e = make_engine(setup["models"])
    try:
        if "focus" in first["method"]:
            e.tracker_create()
            e.focus_create()
        call = Call(e, setup["frames"], first)
        then = Call(e, setup["frames"], other, like=call)
        assert _stats(e) == (0, 0, 0, 0)
        seen = []
        for _ in range(3):
            call()
            seen.append(_stats(e))
        print(f"{first['method']}: {seen}")
        assert seen == [(n, n, 0, 0), (n, n, n, 0), (n, n, n, n)]
        m = 3 if not other["method"].endswith("_device") else 1
        then()
        after = _stats(e)
        print(f"then {other['method']}: {after}")
        assert after == (n + m, n + m, n, n), "the other entry point must run eagerly under entries of its own"
        call()
        assert _stats(e) == (n + m, n + m, n, 2 * n), "the first entry point's steps must replay behind the other's call"
    finally:
        e.close()
