"""CPU tests of crop quality (include/litepi.h, lp_quality): lp_quality_measure against the NumPy restatement of the rule
(tests/quality_ref.py) bit for bit, the blur property the GPU tests rely on, the record layout and the exported symbols, the
inventory's restatement under the sharpness rank, the option handling of HybridPipeline and the CLI, and the shared rule header
under sanitizers as a stand-alone program.  No device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import inventory_ref as I
import quality_ref as Q
import tracking_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lp_quality_enable", "lp_quality_buffer", "lp_quality_read", "lp_quality_measure", "lp_inventory_set_rank", "lp_test_quality")
SIZES = (4, 8, 36, 64, 188, 224, 372)


def _lib():
    from litepi import _ffi
    return _ffi.load_library()


# ---------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("S", SIZES)
def test_quality_measure_equals_the_rule_bit_for_bit(S):
    from litepi import backend
    for name, crop in Q.shared_crops(S).items():
        got, want = backend.quality_measure(crop), Q.measure(crop)
        assert got.tobytes() == want.tobytes(), (S, name, got, want)
        assert got["flags"] == Q.VALID and not got["reserved"].any()
    z, o, cb = (backend.quality_measure(Q.extreme_crops(S)[k]) for k in ("zeros", "ones", "checkerboard"))
    assert (z["sharpness"], z["luma_mean"], z["luma_var"], z["clip_lo"], z["clip_hi"]) == (0, 0, 0, 1, 0)
    assert (o["sharpness"], o["luma_mean"], o["luma_var"], o["clip_lo"], o["clip_hi"]) == (0, 255, 0, 0, 1)
    assert cb["sharpness"] == np.float32(1040400.0) and cb["luma_mean"] == np.float32(127.5) and cb["luma_var"] == np.float32(16256.25)
    assert cb["clip_lo"] == 0.5 and cb["clip_hi"] == 0.5


def test_largest_sharpness_needs_the_int64_products():
    from litepi import backend
    s = Q.sums(Q.checkerboard_crop(224))
    assert s["s1"] == 0 and s["s2"] == 222 * 222 * 1020 * 1020 > 2 ** 32 and s["n"] * s["s2"] > 2 ** 50
    assert backend.quality_measure(Q.checkerboard_crop(224))["sharpness"] == np.float32(1040400.0)


def test_odd_and_smallest_sizes():
    from litepi import backend
    for S in (3, 5, 7, 33):   # the host rule takes any S in 3..1024
        crop = Q.noise_crop(S, 3)
        assert backend.quality_measure(crop).tobytes() == Q.measure(crop).tobytes(), S


@pytest.mark.parametrize("S", (8, 36, 64, 224))
def test_a_box_blur_lowers_the_sharpness_strictly(S):
    """the property the inventory tests rely on, for the seeded crops they use"""
    for crop in (Q.noise_crop(S, 0), Q.noise_crop(S, 1), Q.sign_crop(S)):
        b1 = Q.box_blur(crop)
        b2 = Q.box_blur(b1)
        s0, s1, s2 = (float(Q.measure(c)["sharpness"]) for c in (crop, b1, b2))
        assert s0 > s1 > s2 > 0, (S, s0, s1, s2)


def test_quality_measure_refuses_bad_arguments():
    from litepi import _ffi, backend
    lib = _lib()
    crop = Q.noise_crop(8)
    out = _ffi.LpQuality()
    assert lib.lp_quality_measure(crop.ctypes.data, 8, C.byref(out)) == 0 and out.flags == 1
    for args in ((None, 8, C.byref(out)), (crop.ctypes.data, 8, None), (crop.ctypes.data, 2, C.byref(out)), (crop.ctypes.data, 1025, C.byref(out)),
                 (crop.ctypes.data, 0, C.byref(out)), (crop.ctypes.data, -4, C.byref(out))):
        assert lib.lp_quality_measure(*args) == _ffi.LP_ERR_ARG, args[1]
        assert lib.lp_last_error()
    for bad in (np.zeros((8, 6, 3), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8)):
        with pytest.raises(ValueError):
            backend.quality_measure(bad)
    with pytest.raises(_ffi.LitepiError):
        backend.quality_measure(np.zeros((2, 2, 3), np.uint8))


# ---------------------------------------------------------------------------- layout and exports
def test_layout_and_exports():
    from litepi import _ffi
    lib = _lib()
    assert C.sizeof(_ffi.LpQuality) == 32 and np.dtype(_ffi.QUALITY_DTYPE).itemsize == 32 and np.dtype(Q.QUALITY_DTYPE) == np.dtype(_ffi.QUALITY_DTYPE)
    offs = {n: getattr(_ffi.LpQuality, n).offset for n, *_ in _ffi.LpQuality._fields_}
    assert offs == dict(sharpness=0, luma_mean=4, luma_var=8, clip_lo=12, clip_hi=16, flags=20, reserved=24)
    assert {n: np.dtype(_ffi.QUALITY_DTYPE).fields[n][1] for n in offs} == offs
    assert (_ffi.LP_QUALITY_VALID, _ffi.LP_RANK_CONFIG, _ffi.LP_RANK_SHARPNESS) == (Q.VALID, Q.RANK_CONFIG, Q.RANK_SHARPNESS) == (1, 0, 1)
    header = open(os.path.join(ROOT, "include", "litepi.h")).read()
    declared = set(re.findall(r"\b(lp_[a-z0-9_]+)\s*\(", header))
    assert "#define LP_QUALITY_VALID 1" in header and "LP_RANK_CONFIG = 0, LP_RANK_SHARPNESS = 1" in header
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} is not declared in include/litepi.h"
        assert s in _ffi.SYMBOLS and hasattr(lib, s) and getattr(lib, s).restype is C.c_int
    assert lib.lp_version() == 310 == _ffi.ABI_VERSION
    e = Q.empty_records(2)
    assert Q.is_empty(e).all() and e.tobytes() == (np.float32(-1).tobytes() + bytes(28)) * 2 and not Q.is_empty(np.array([Q.measure(Q.noise_crop(8))]))[0]


# ---------------------------------------------------------------------------- the inventory's restatement under the rank
def _one_track(n_frames, max_det=4):
    dets, tracks = np.zeros((n_frames, max_det), dtype=R.DET_DTYPE), np.zeros((n_frames, max_det), dtype=R.TRACK_DTYPE)
    for f in range(n_frames):   # the box grows every frame
        dets[f, 0] = (100.0 - 2 * f, 80.0 - 2 * f, 140.0 + 2 * f, 120.0 + 2 * f, 0.9, 0, 5, 0.8)
        tracks[f, 0]["track_id"], tracks[f, 0]["slot"], tracks[f, 0]["hits"] = 1, 0, f + 1
    return dets, tracks, np.ones(n_frames, np.int32)


def test_sharpness_rank_ref_keeps_the_last_sharp_frame():
    S = 8
    sign = Q.sign_crop(S)
    blur2 = Q.box_blur(Q.box_blur(sign))
    dets, tracks, counts = _one_track(6)
    crops = {(f, 0): (sign if f < 4 else blur2) for f in range(6)}
    quality = Q.records_for([crops[(f, 0)] for f in range(6)], list(range(6)), [0] * 6, 6, 4)
    by_area, by_sharp = (Q.InventorySharpRef(max_det=4, track_cfg=dict(max_tracks=4), crop_size=S) for _ in range(2))
    by_area.feed(dets, tracks, counts, crops=crops)
    by_sharp.feed(dets, tracks, counts, crops=crops, quality=quality)
    a, s = by_area.open()[0], by_sharp.open()[0]
    assert a["best_frame"] == 5 and s["best_frame"] == 0   # equal sharpness over frames 0..3: the tie keeps the earlier sighting
    assert s["best_quality"].tobytes() == Q.measure(sign)["sharpness"].tobytes()
    assert (s["x1"], s["x2"]) == (dets[0, 0]["x1"], dets[0, 0]["x2"]) and by_sharp.best == I.BEST_AREA
    # an unmeasured first sighting is replaced by the first measured one; a later unmeasured one never replaces
    q2 = quality.copy()
    q2[0] = Q.empty_records(4)
    q2[3] = Q.empty_records(4)
    ref = Q.InventorySharpRef(max_det=4, track_cfg=dict(max_tracks=4), crop_size=S)
    ref.feed(dets[:1], tracks[:1], counts[:1], crops={}, quality=q2[:1])
    assert ref.open()[0]["best_frame"] == 0 and ref.open()[0]["best_quality"] == -1 and not ref.open()[0]["flags"] & I.HAS_CROP
    ref.feed(dets[1:], tracks[1:], counts[1:], crops={(f - 1, 0): c for (f, _), c in crops.items() if f not in (0, 3)}, quality=q2[1:])
    assert ref.open()[0]["best_frame"] == 1 and ref.open()[0]["flags"] & I.HAS_CROP


# ---------------------------------------------------------------------------- options
def test_inventory_config_knows_no_sharpness():
    from litepi import _ffi, backend
    with pytest.raises(ValueError):
        backend.inventory_config(best="sharpness")
    with pytest.raises(ValueError):
        backend.inventory_config(best="biggest")
    assert "sharpness" not in backend.INVENTORY_BEST and 3 not in backend.INVENTORY_BEST.values()
    c = backend.inventory_config()
    c.best = 3
    assert backend.inventory_config_check(c) == _ffi.LP_ERR_ARG   # the struct cannot carry a fourth value


def test_pipeline_resolves_sharpness_outside_the_config():
    from litepi import _ffi, backend
    on, rank, inv = backend.check_quality_options(False, dict(best="sharpness", max_signs=10))
    assert (on, rank, inv) == (True, "sharpness", dict(max_signs=10))
    assert backend.inventory_config(**inv).best == _ffi.LP_BEST_AREA   # the config keeps its default best
    assert backend.check_quality_options(False, True) == (False, "config", {})
    assert backend.check_quality_options(True, dict(best="area")) == (True, "config", dict(best="area"))
    assert backend.check_quality_options(False, None) == (False, "config", {})
    with pytest.raises(ValueError) as ei:
        backend.check_quality_options(False, dict(best="sharpness", keep_crops=0))
    assert "keep_crops" in str(ei.value)
    with pytest.raises(ValueError) as ei:   # refused before any model file is opened
        backend.HybridPipeline("no_such.param", "no_such.bin", "no_such.pth", "shufflenetv2", track=True,
                               inventory=dict(best="sharpness", keep_crops=0))
    assert "sharpness" in str(ei.value)
    with pytest.raises(ValueError):   # an unknown name still reaches inventory_config's refusal... before anything is loaded
        backend.inventory_config(**backend.check_quality_options(False, dict(best="biggest"))[2])
    assert backend.INVENTORY_RANKS == dict(config=0, sharpness=1) and backend.QUALITY_RESULT_KEYS == ("sharpness", "luma_mean", "clip_lo", "clip_hi")


def test_cli_quality_arguments(tmp_path):
    from litepi import e2e
    raw = tmp_path / "f.bgr"   # two packed BGR frames: the accepted argument sets are checked against a real sequence
    raw.write_bytes(bytes(2 * 64 * 64 * 3))
    base = ["--raw_frames", str(raw), "--frame_size", "64x64"]
    a = e2e.build_parser().parse_args([])
    assert a.quality is False and a.inventory_best == "area" and not e2e.quality_wanted(a)
    a = e2e.build_parser().parse_args(base + ["--track", "--inventory", "--inventory_best", "sharpness"])
    e2e.check_frame_args(a)
    assert a.quality is False and e2e.quality_wanted(a)   # implied
    a = e2e.build_parser().parse_args(base + ["--track", "--quality"])
    e2e.check_frame_args(a)
    assert e2e.quality_wanted(a)
    assert not e2e.quality_wanted(e2e.build_parser().parse_args(base + ["--track", "--inventory", "--inventory_best", "cls_conf"]))
    for extra, word in ((["--quality"], "--track"), (["--inventory_best", "sharpness"], "--inventory"),
                        (["--track", "--inventory_best", "sharpness"], "--inventory")):
        args = e2e.build_parser().parse_args(base + extra)
        with pytest.raises(SystemExit) as ei:
            e2e.check_frame_args(args)
        assert word in str(ei.value) and ("--quality" in str(ei.value) or "sharpness" in str(ei.value)), extra
    with pytest.raises(SystemExit):
        e2e.build_parser().parse_args(["--inventory_best", "biggest"])
    assert e2e.QUALITY_CSV_COLUMNS == ("sharpness", "luma_mean", "clip_lo", "clip_hi")
    assert e2e.TRACKS_CSV_COLUMNS[-1] == "confirmed"   # the columns are appended, nothing moves


# ---------------------------------------------------------------------------- the shared header under sanitizers
def test_quality_measure_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "quality_measure_check")
    src = os.path.join(ROOT, "tests", "native", "quality_measure_check.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK" and lines[-2].startswith("crops ") and lines[-2].endswith("largest sharpness 1040400.0")
    assert lines[-3].startswith("strip walks ")
