"""The letterbox core (csrc/letterbox_core.h) on the CPU: tests/native/letterbox_core_check.cpp, a stand-alone program built
with a plain g++ under AddressSanitizer and UBSan, plays the workgroups of the staged form and the per-pixel form through the
header on frames that end with their heap block (see its header comment for what it checks itself), and dumps every picture;
the dumps are compared here, byte for byte, with the references the GPU tests trust: views_ref.make_view for the windows,
rect_ref.letterbox for the rectangular letterbox, evidence_ref.picture for the evidence geometry.  No device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import evidence_ref
import rect_ref as RR
import views_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the frames and window lists of test_gpu_views.GATHER at both sizes (with the 11.25x window that the row rule sends to the
# per-pixel form); rectangular letterboxes, the 3x and 4.6x down-scales on frames cut to 96 source rows; evidence pictures
RECT = [((224, 416), (37, 100)), ((224, 416), (100, 4480)), ((384, 640), (96, 1920)), ((384, 640), (96, 2944))]
EVIDENCE_FRAME = (750, 900)
EVIDENCE_WINDOWS = [(5, 3, 16, 16), (101, 57, 200, 200), (77, 21, 800, 720)]


def _cases(d):
    """writes the frames and cases.txt into d; returns {name: expected picture}"""
    import test_gpu_views as G
    want, lines, frames = {}, [], {}

    def frame(key, shape, seed):
        if key not in frames:
            img = np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)
            img.tofile(os.path.join(d, key + ".raw"))
            frames[key] = img
        return frames[key]

    def add(name, kind, key, img, win, oh, ow, g, exp):
        H, W = img.shape[:2]
        lines.append(" ".join(str(v) for v in (name, kind, key + ".raw", H, W, *win, oh, ow, g["new_w"], g["new_h"], g["top"], g["left"])))
        assert exp.shape == (oh, ow, 3) and exp.dtype == np.uint8
        want[name] = exp

    for shape, s in G.GATHER_CASES:
        img = frame(f"gather_{shape[0]}x{shape[1]}_{s}", shape, shape[0] * 7 + s)
        for k, v in enumerate(G.GATHER[shape]):
            add(f"gather_{shape[0]}x{shape[1]}_S{s}_v{k}", "tile", f"gather_{shape[0]}x{shape[1]}_{s}", img, V.window(v, *shape), s, s,
                V.view_geometry(s, *shape, v), V.make_view(img, s, v)[0])
    for (sh, sw), hw in RECT:
        img = frame(f"rect_{hw[0]}x{hw[1]}", hw, hw[0] * 7 + hw[1] + sh)
        add(f"rect_{hw[0]}x{hw[1]}_into_{sh}x{sw}", "tile", f"rect_{hw[0]}x{hw[1]}", img, (0, 0, hw[1], hw[0]), sh, sw,
            RR.letterbox_geometry(sh, sw, *hw), RR.letterbox(img, sh, sw)[0])
    img = frame("evidence", EVIDENCE_FRAME, 11)
    for E in (32, 64):
        for k, win in enumerate(EVIDENCE_WINDOWS):
            add(f"evidence_E{E}_w{k}", "evid", "evidence", img, win, E, E, V.view_geometry(E, *EVIDENCE_FRAME, win), evidence_ref.picture(img, E, win))
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return want


def test_letterbox_core_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "letterbox_core_check")
    src = os.path.join(ROOT, "tests", "native", "letterbox_core_check.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True, timeout=300)
    d = str(tmp_path)
    want = _cases(d)
    r = subprocess.run([exe, d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK" and lines[-2].startswith(f"cases {len(want)} staged "), lines[-2:]
    form = {ln.split(":")[0]: ln.split(": ")[1] for ln in lines if ": " in ln}
    # the forms the device's rules take: the 11.25x window, the 10.8x letterbox and the 800-pixel evidence window per pixel
    per_pixel = sorted(n for n, f in form.items() if f == "per-pixel only")
    assert per_pixel == sorted(["gather_70x720_S64_v0", "gather_70x720_S64_v5", "rect_100x4480_into_224x416", "evidence_E32_w2", "evidence_E64_w2"]), per_pixel
    assert all(f.startswith("staged, ") for n, f in form.items() if n not in per_pixel) and len(form) == len(want)
    for name, exp in want.items():
        got = np.fromfile(os.path.join(d, name + ".bin"), dtype=np.uint8)
        assert got.size == exp.size, name
        got = got.reshape(exp.shape)
        assert np.array_equal(got, exp), f"{name}: {int((got != exp).sum())} bytes differ, first at {np.argwhere(got != exp)[0].tolist()}"
