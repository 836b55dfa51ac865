"""The geometry of the two fused network-head kernels (csrc/stem_walk.h: row-wise staging of the uint8 tile, the stem walks'
incremental LDS offsets) without a device.

tests/native/stem_walk_check.cpp includes the header alone, built with a plain g++ under -fsanitize=address,undefined.  For both
geometries (stem_block_kernel's pixel pairs, stem_block16_kernel<8>'s pixels) and every wave, lane and iteration it checks that the
incremental read and write offsets equal the closed forms, that every LDS read (with the two further dwords of the gather) lies
inside in_tile and every write inside st_tile, and that the peeled iterations are exactly those in which some lane is not live.
For the staging it checks, on 640 x 640, 352 x 352 (partial tiles both ways), 384 x 640 and 64 x 64 (every tile touches a border)
and every tile of each, that the (row, dword) -> image-dword-or-zero map equals "row r = image row 4 oy0 - 3 + r, dword c = row
dword w0 + c, zero outside" and that every loaded image dword lies inside the image."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("stem_walk") / "stem_walk_check")
    src = os.path.join(ROOT, "tests", "native", "stem_walk_check.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", inc, src,
                    "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def test_walks_and_staging_hold(report):
    assert report[-1].startswith("ok ") and int(report[-1].split()[1]) > 1_000_000, report[-3:]


def test_one_peeled_iteration_per_walk(report):
    # 9 iterations per wave in both kernels; only the last can hold a lane beyond the tile's last pair / pixel
    assert "pair_walk iters 9 full 8" in report and "pixel_walk iters 9 full 8" in report, report[:2]


def test_every_tile_of_every_size_was_staged(report):
    # ceil(W2 / 32) x ceil(H2 / 8) tiles of the stride-4 output
    want = {"640x640": 5 * 20, "352x352": 3 * 11, "384x640": 5 * 12, "64x64": 1 * 2}
    got = {ln.split()[1]: int(ln.split()[3]) for ln in report if ln.startswith("stage ")}
    assert got == want
