"""The host logic of the decoder-surface front (csrc/surface_plan.h) and of the plan rings (csrc/ring_slots.h) without a device or Python in the loop.

tests/native/surface_plan_check.cpp includes the two headers alone, built with a plain g++ under -fsanitize=address,undefined: the
argument rules of include/litepi.h on exact-sized arrays, the converter's table records (pitches resolved, the `aligned` flag,
max_blocks) for 2000 seeded surface sets, and the slot policy of the pinned rings against a model of the copies in flight."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_surface_plan_header_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "surface_plan_check")
    src = os.path.join(ROOT, "tests", "native", "surface_plan_check.cpp")
    inc = os.path.join(ROOT, "yolo-litepi_amd", "csrc")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", inc, src, "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK" and lines[0].startswith("rules ") and lines[1].startswith("tables ") and lines[2] == "ring 992 waits in 1000 calls"
